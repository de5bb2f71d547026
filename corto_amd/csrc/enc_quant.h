// enc_quant.h — the encoder's per-element quantisation recipes, shared by k_enc_quantize (k_encode.hip) and
// k_enc_quantize_batch / k_enc_est_normal (k_encode_batch.hip) - the one recipe table of the device encoders.  Upstream's float
// operations one by one (no FMA: the library is built with -ffp-contract=off; IEEE divide); (int) is x86's cvttss2si / cvttsd2si:
// INT_MIN when out of range.
#pragma once
#include "kernels_common.h"
#include "device_plan.h"
#include "../../include/corto_hip.h"

namespace corto_hip {

__device__ __forceinline__ void enc_to_octa(float vx, float vy, float vz, int32_t unit, int32_t o[2]) {   // normal_attribute.h:75-85
	float s = fabsf(vx) + fabsf(vy); s = s + fabsf(vz);
	float px = vx/s, py = vy/s;
	if(vz < 0) {
		const float qx = 1.0f - fabsf(py), qy = 1.0f - fabsf(px);
		px = qx; py = qy;
		if(vx < 0) px = -px;
		if(vy < 0) py = -py;
	}
	o[0] = f2i_x86(px*(float)unit); o[1] = f2i_x86(py*(float)unit);
}

__device__ __forceinline__ void enc_quantize_color(const uint8_t *c, uint8_t *o, const QuantJob &J) {
	uint8_t y[4] = {0, 0, 0, 0};
	for(uint32_t k = 0; k < J.N && k < 4; k++) y[k] = (uint8_t)(c[k]/J.qc[k]);
	const uint8_t ycc[4] = {y[1], (uint8_t)(y[2] - y[1]), (uint8_t)(y[0] - y[1]), y[3]};
	for(uint32_t k = 0; k < J.N && k < 4; k++) o[k] = ycc[k];
}

// element i of a job that reads through a crthip_mesh_layout (a stride, an origin, int16 normals): the array is read where it lies, one
// element a lane, and the recipe behind the load is enc_quantize_one's.  The conversions are upstream's single float operations:
// input - o (src/encoder.cpp:80-81), (float)v/32767.0f (:156).
__device__ __forceinline__ void enc_quantize_one_layout(const QuantJob &J, uint32_t i) {
	const uint8_t *base = (const uint8_t *)J.in;
	if(J.kind == QK_NORMAL) {
		const bool i16 = (J.flags & QF_NORMAL_I16) != 0;
		const uint8_t *p = base + (size_t)i*(J.stride ? J.stride : i16 ? 6u : 12u);
		float v[3];
		if(i16) { const int16_t *s = (const int16_t *)p; for(int k = 0; k < 3; k++) v[k] = (float)s[k]/32767.0f; }
		else { const float *f = (const float *)p; for(int k = 0; k < 3; k++) v[k] = f[k]; }
		enc_to_octa(v[0], v[1], v[2], J.unit, (int32_t *)J.out + (size_t)i*2);
		return;
	}
	if(J.kind == QK_COLOR) {
		enc_quantize_color(base + (size_t)i*(J.stride ? J.stride : J.N), (uint8_t *)J.out + (size_t)i*J.N, J);
		return;
	}
	const uint32_t n = J.comps ? J.comps : 1u, v = i/n, c = i - v*n;
	const uint32_t esize = J.kind == QK_DOUBLE ? 8u : J.kind == QK_INT ? (J.format == CRTHIP_FMT_INT8 ? 1u : J.format == CRTHIP_FMT_INT16 ? 2u : 4u) : 4u;
	const uint8_t *p = base + (size_t)v*(J.stride ? J.stride : n*esize) + (size_t)c*esize;
	int32_t *o = (int32_t *)J.out + i;
	if(J.kind == QK_FLOAT) {
		const float x = *(const float *)p - ((J.flags & QF_ORIGIN) ? J.origin[c < 3 ? c : 0] : 0.0f);
		*o = f2i_x86(x/J.q);
	} else if(J.kind == QK_INT) {
		const int32_t w = J.format == CRTHIP_FMT_INT8 ? (int32_t)*(const int8_t *)p : J.format == CRTHIP_FMT_INT16 ? (int32_t)*(const int16_t *)p : *(const int32_t *)p;
		*o = f2i_x86((float)w/J.q);
	} else *o = d2i_x86(*(const double *)p/(double)J.q);
}

// element i of job J: GENERIC (int)(x/q) for every input format (vertex_attribute.h:79-104): float and the integers divide in float
// (an int32 beyond 2^24 rounds to nearest even on its way to float, as cvtsi2ss does), a double divides in double and truncates
// like cvttsd2si; NORMAL toOcta; COLOR byte/qc then (g, b - g, r - g, a) (color_attribute.cpp:30-44, point.h:213)
__device__ __forceinline__ void enc_quantize_one(const QuantJob &J, uint32_t i) {
	if(J.stride | J.flags) { enc_quantize_one_layout(J, i); return; }
	if(J.kind == QK_FLOAT) {
		const float x = ((const float *)J.in)[i] - 0.0f;
		((int32_t *)J.out)[i] = f2i_x86(x/J.q);
	} else if(J.kind == QK_INT) {
		const int32_t v = J.format == CRTHIP_FMT_INT8 ? (int32_t)((const int8_t *)J.in)[i]
		                : J.format == CRTHIP_FMT_INT16 ? (int32_t)((const int16_t *)J.in)[i] : ((const int32_t *)J.in)[i];
		((int32_t *)J.out)[i] = f2i_x86((float)v/J.q);
	} else if(J.kind == QK_DOUBLE) {
		const double x = ((const double *)J.in)[i];
		((int32_t *)J.out)[i] = d2i_x86(x/(double)J.q);
	} else if(J.kind == QK_NORMAL) {
		const float *v = (const float *)J.in + (size_t)i*3;
		enc_to_octa(v[0], v[1], v[2], J.unit, (int32_t *)J.out + (size_t)i*2);
	} else enc_quantize_color((const uint8_t *)J.in + (size_t)i*J.N, (uint8_t *)J.out + (size_t)i*J.N, J);
}

} // namespace corto_hip
