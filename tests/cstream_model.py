"""A direct restatement of the reference's value coders (include/corto/cstream.h, src/bitstream.cpp) in plain Python: what
crthip_encode_values' bit words and width arrays are compared with (tests/test_gpu_parity.py, the encode size-class modules)."""
import numpy as np


def model_bits(fields):
    """MSB-first bit writer (src/bitstream.cpp:86-101): fields = iterable of (value, nbits) -> uint32 words"""
    acc, nb, words = 0, 0, []
    for v, n in fields:
        acc = (acc << n) | (int(v) & ((1 << n) - 1)); nb += n
        while nb >= 32:
            words.append((acc >> (nb - 32)) & 0xFFFFFFFF); nb -= 32; acc &= (1 << nb) - 1
    if nb:
        words.append((acc << (32 - nb)) & 0xFFFFFFFF)
    return np.array(words, dtype=np.uint32)


def model_array(a):
    """OutStream::encodeArray<int> (include/corto/cstream.h:143-164): one width per element -> (words, [logs])"""
    def needed(x):
        x = int(x)
        if x == 0: return 0
        if x == -1: return 1
        if x < 0: x = -x - 1
        return 1 + x.bit_length()
    logs = np.array([max(needed(x) for x in row) for row in a], dtype=np.uint8)
    fields = [(int(x) + (1 << (int(d) - 1)), int(d)) for row, d in zip(a, logs) if d for x in row]
    return model_bits(fields), [logs]


def model_values(a):
    """OutStream::encodeValues (include/corto/cstream.h:115-141): component-major, one width per value, sign folded"""
    logs, fields = [], []
    for c in range(a.shape[1]):
        lg = np.zeros(len(a), dtype=np.uint8)
        for i, x in enumerate(a[:, c]):
            x = int(x)
            if x == 0: continue
            r = abs(x).bit_length()
            lg[i] = r
            fields.append((x if x > 0 else -x - (1 << (r - 1)), r))
        logs.append(lg)
    return model_bits(fields), logs


def expected_stream(words, blocks):
    """one stream of crthip_encode_values: "u32 nwords | words | blocks" """
    return np.array([len(words)], dtype="<u4").tobytes() + words.astype("<u4").tobytes() + b"".join(bytes(b) for b in blocks)
