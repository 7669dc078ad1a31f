// g711.hpp -- G.711 A-law / mu-law arithmetic on the device (Snack_* of the reference's g711.c), shared by the streaming
// converters (codec.hip), the bridge's fused tick (bridge.hip) and the per-leg concealer's RECEIVED pass (plc.hip).  All integer,
// bit-exact.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/msmi355x.h"

namespace {

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ us2 as_us2(uint32_t v) { return __builtin_bit_cast(us2, v); }
__device__ __forceinline__ uint32_t as_u32(us2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ us2 splat(unsigned short v) { return us2{v, v}; }

// two A-law codes (one per 16-bit half, 0..255) -> two int16 samples.  g711.c:147-166
__device__ __forceinline__ uint32_t alaw2lin_x2(uint32_t codes) {
	const us2 a = as_us2(codes ^ 0x00550055u);
	const us2 seg = (a >> splat(4)) & splat(7);
	const us2 lin = __builtin_elementwise_min(seg, splat(1));      // 0 in the first (linear) segment, else 1
	const us2 mant = ((a & splat(15)) << splat(4)) + splat(8) + (lin << splat(8)); // +8, or +0x108
	const us2 mag = mant << (seg - lin);                            // seg 0,1: no shift; seg k: k-1
	const us2 neg = ((a >> splat(7)) & splat(1)) ^ splat(1);       // sign bit SET means positive
	const us2 m = splat(0) - neg;                                   // 0xFFFF where negative
	return as_u32((mag ^ m) + neg);
}

// two mu-law codes -> two int16 samples.  g711.c:242-255
__device__ __forceinline__ uint32_t ulaw2lin_x2(uint32_t codes) {
	const us2 u = as_us2(codes ^ 0x00ff00ffu);
	const us2 mag = ((((u & splat(15)) << splat(3)) + splat(0x84)) << ((u >> splat(4)) & splat(7))) - splat(0x84);
	const us2 neg = (u >> splat(7)) & splat(1);
	const us2 m = splat(0) - neg;
	return as_u32((mag ^ m) + neg);
}

// g711.c:113-141: 13-bit magnitude, segment = position of the leading one
__device__ __forceinline__ uint32_t lin2alaw(int pcm) {
	int v = pcm >> 3;
	const int sign = v >> 31; // -1 for negative input
	v ^= sign;                // -v - 1
	const int seg = max(27 - __clz(v), 0); // bit_length - 5; v <= 4095 so seg <= 7
	const int mant = (v >> max(seg, 1)) & 15;
	return (uint32_t)(((seg << 4) | mant) ^ (0xD5 ^ (sign & 0x80)));
}

// g711.c:200-231: 14-bit magnitude clipped at 8159, bias 33; the clipped maximum overflows the table (seg 8)
__device__ __forceinline__ uint32_t lin2ulaw(int pcm) {
	int v = pcm >> 2;
	const int sign = v >> 31;
	v = min((v ^ sign) - sign, 8159) + 33;
	const int seg = max(26 - __clz(v), 0); // bit_length - 6
	const int code = seg >= 8 ? 0x7F : ((seg << 4) | ((v >> (seg + 1)) & 15));
	return (uint32_t)(code ^ (0xFF ^ (sign & 0x80)));
}

// ---- a leg's codec as data (mi_bridge_create_legs): `row` is the leg's byte row, whose pitch is a multiple of 16.
// bridge.hip's load_group with the kind in a register, in two steps so that a lane's loads are all issued before the first is used:
// one 16-byte load whatever the kind -- a PCM leg's group, or the aligned pair of 8-byte groups that holds a G.711
// leg's --, then both laws' decodes of the 8 code bytes and selects.  No branch: the lanes of a wavefront hold up to
// eight members, of all three kinds.
__device__ __forceinline__ uint4 load_raw_leg(const uint8_t *row, int kind, int g) {
	return *reinterpret_cast<const uint4 *>(row + 16 * (kind == MI_SESSION_PCM16 ? g : g >> 1));
}

__device__ __forceinline__ uint4 decode_group_leg(uint4 v, int kind, int g) {
	const bool pcm = kind == MI_SESSION_PCM16, mu = kind == MI_SESSION_PCMU;
	const uint32_t w[2] = {(g & 1) ? v.z : v.x, (g & 1) ? v.w : v.y};
	uint32_t o[4];
#pragma unroll
	for (int k = 0; k < 2; ++k) {
		const uint32_t lo = __builtin_amdgcn_perm(0u, w[k], 0x0c010c00u), hi = __builtin_amdgcn_perm(0u, w[k], 0x0c030c02u);
		const uint32_t alo = alaw2lin_x2(lo), ahi = alaw2lin_x2(hi), ulo = ulaw2lin_x2(lo), uhi = ulaw2lin_x2(hi);
		o[2 * k] = mu ? ulo : alo;
		o[2 * k + 1] = mu ? uhi : ahi;
	}
	return make_uint4(pcm ? v.x : o[0], pcm ? v.y : o[1], pcm ? v.z : o[2], pcm ? v.w : o[3]);
}

} // namespace
