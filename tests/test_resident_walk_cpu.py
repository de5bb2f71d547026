"""The device walk of blobs that live only in device memory (crt_walk.h, run by k_walk.hip) against the host walk (crt_format.cpp's
walk_blob), on the host: tests/cpp/walk_probe.cpp runs the walker through a reader that counts every read at or past the blob's length,
turns the record back into a layout with the library's record_to_layout and compares status and layout with walk_blob's.  Identical status
everywhere, identical layouts wherever the walk succeeds, no read outside the blob, no record byte written past its capacity.  No GPU."""
import os
import subprocess

import pytest

import resident_corpus as rc

ROOT = rc.ROOT
CSRC = os.path.join(ROOT, "corto_amd", "csrc")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("walk_probe")
    exe = os.path.join(str(d), "walk_probe")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O2", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "walk_probe.cpp"),
                           os.path.join(CSRC, "crt_format.cpp"), "-o", exe])
    blobs = rc.corpus()
    path = os.path.join(str(d), "corpus.bin")
    rc.write_corpus(path, [b for _, b in blobs])
    names = [n for n, _ in blobs]

    def run(cap, *cmd):
        out = subprocess.run([exe, path, str(cap)] + [str(c) for c in cmd], check=True, capture_output=True, text=True, timeout=600).stdout
        lines = out.strip().splitlines()
        res = dict(kv.split("=", 1) for kv in lines[-1].split())
        codes = {int(k): int(v) for k, v in (c.split(":") for c in res.pop("codes").split(",") if c)}
        res = {k: int(v) for k, v in res.items()}
        res["codes"] = codes
        res["lines"] = lines[:-1]
        return res
    run.names = names
    return run


def clean(r):
    assert r["mismatch"] == 0, [x for x in r["lines"] if x.startswith("MISMATCH")]
    assert r["oob"] == 0, "the walker asked for bytes past a blob's end"
    assert r["guard"] == 0, "a record was written past its capacity"


def test_golden_blobs_walk_identically(probe):
    r = probe(1024, "golden")
    clean(r)
    n = len(probe.names)
    assert r["n"] == n and r["codes"] == {0: n}
    # what a record cannot hold goes to the host walk (blobs with many generic attributes, kilobytes of exif); nothing else does: every
    # fixture, C4 and non-lattice blob fits
    back = [probe.names[int(line.split()[-1])] for line in r["lines"] if line.startswith("FALLBACK")]
    assert len(back) == r["fallback"] and r["ok"] == n - r["fallback"]
    assert {"big_exif", "many_streams"} <= set(back), back
    assert all(b in ("big_exif", "many_streams") or b.startswith("generic_inputs:") for b in back), back


@pytest.mark.parametrize("cap", [64, 256, 512])
def test_small_record_capacities(probe, cap):
    """a record too small for most blobs: every overflow is flagged (and then walked on the host), nothing is written past the record"""
    r = probe(cap, "golden")
    clean(r)
    assert r["fallback"] + r["ok"] == r["n"]
    if cap == 64:
        assert r["fallback"] == r["n"]
    else:
        assert 0 < r["fallback"] < r["n"]


@pytest.mark.parametrize("name", ["fields31", "cone_fan", "radius_attr", "entropy_none", "crafted:group_props"])
def test_every_truncation(probe, name):
    i = probe.names.index(name)
    r = probe(1024, "trunc", i)
    clean(r)
    assert r["codes"].get(0) == 1 and r["codes"].get(-3, 0) > 0 and r["codes"].get(-2, 0) == 4
    r = probe(128, "trunc", i)
    clean(r)


@pytest.mark.parametrize("name", ["c4_unit", "entropy_none", "group_props", "two_groups", "nrm_estimated_rgb", "cloud_diff",
                                  "generic_formats:crt_sphere_q3", "crafted:c4_unit"])
def test_header_and_framing_edits(probe, name):
    i = probe.names.index(name)
    r = probe(1024, "edits", i)
    clean(r)
    assert r["n"] > 300
    assert {0, -2, -3}.issubset(r["codes"]), r["codes"]


def test_random_corruptions(probe):
    r = probe(1024, "fuzz", 20261016, 12000)
    clean(r)
    assert r["n"] == 12000
    assert len(r["codes"]) >= 4, r["codes"]          # every outcome shows up: ok, truncated, limit, entropy, magic
    r = probe(192, "fuzz", 7, 3000)
    clean(r)
