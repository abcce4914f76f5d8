// la_prep_common.h — chunk I/O of the prologue passes (la_prep_qk.hip, la_prep_v.hip, la_v_prep_tiles in la_prep_fp8.hip): a CHUNK is 8 consecutive elements of a row, one
// 16-byte load or store of 16-bit elements, two of fp32, one 8-byte store of e4m3; between the two everything is fp32. Everything
// sits in the unnamed namespace of the including file and is inlined into its kernels: no symbol, no device code of its own.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace la {
namespace {

typedef unsigned int pq_u32x4 __attribute__((ext_vector_type(4)));
typedef float pq_f32x4 __attribute__((ext_vector_type(4)));
typedef float pq_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int pq_u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 pq_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 pq_bf16x8 __attribute__((ext_vector_type(8)));

template <int DT> struct PrepLoad;         // DT: la_dtype; raw = 8 consecutive elements as loaded (what a lane keeps of a chunk), to_float -> fp32
template <> struct PrepLoad<0> {           // bf16
    typedef pq_u32x4 raw;
    static __device__ __forceinline__ raw zero() { return raw{0u, 0u, 0u, 0u}; }
    static __device__ __forceinline__ raw load(const void* base, int64_t off) {
        return *reinterpret_cast<const pq_u32x4*>(static_cast<const uint16_t*>(base) + off);
    }
    static __device__ __forceinline__ void to_float(const raw& w, float (&x)[8]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i] = __uint_as_float(w[i] << 16);
            x[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        }
    }
};
template <> struct PrepLoad<1> {           // fp16
    typedef pq_f16x8 raw;
    static __device__ __forceinline__ raw zero() { return raw{0, 0, 0, 0, 0, 0, 0, 0}; }
    static __device__ __forceinline__ raw load(const void* base, int64_t off) {
        return *reinterpret_cast<const pq_f16x8*>(static_cast<const uint16_t*>(base) + off);
    }
    static __device__ __forceinline__ void to_float(const raw& w, float (&x)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = static_cast<float>(w[i]);
    }
};
template <> struct PrepLoad<3> {           // fp32
    struct raw { pq_f32x4 a, c; };
    static __device__ __forceinline__ raw zero() { return raw{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}; }
    static __device__ __forceinline__ raw load(const void* base, int64_t off) {
        const float* q = static_cast<const float*>(base) + off;
        return raw{*reinterpret_cast<const pq_f32x4*>(q), *reinterpret_cast<const pq_f32x4*>(q + 4)};
    }
    static __device__ __forceinline__ void to_float(const raw& w, float (&x)[8]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { x[i] = w.a[i]; x[4 + i] = w.c[i]; }
    }
};

template <int DT> struct PrepStore;        // fp32 -> 8 elements, round to nearest even at the store
template <> struct PrepStore<0> {
    static __device__ __forceinline__ void store8(void* base, int64_t off, const float (&y)[8]) {
        pq_bf16x8 w;
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = static_cast<__bf16>(y[i]);
        *reinterpret_cast<pq_bf16x8*>(static_cast<uint16_t*>(base) + off) = w;
    }
};
template <> struct PrepStore<1> {
    static __device__ __forceinline__ void store8(void* base, int64_t off, const float (&y)[8]) {
        pq_f16x8 w;
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = static_cast<_Float16>(y[i]);
        *reinterpret_cast<pq_f16x8*>(static_cast<uint16_t*>(base) + off) = w;
    }
};
// 8 values inside +-448 or NaN (the caller clamps) -> their 8 e4m3 bytes, element i in byte i: the hardware's round to nearest even
__device__ __forceinline__ pq_u32x2 e4m3_pack8(const float (&y)[8]) {
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], hi, true);
    return pq_u32x2{static_cast<unsigned>(lo), static_cast<unsigned>(hi)};
}
template <> struct PrepStore<2> {           // e4m3: y is inside +-448 or NaN (the caller clamps); 8 bytes, one 8-byte store
    static __device__ __forceinline__ void store8(void* base, int64_t off, const float (&y)[8]) {
        *reinterpret_cast<pq_u32x2*>(static_cast<uint8_t*>(base) + off) = e4m3_pack8(y);
    }
};
template <> struct PrepStore<3> {           // fp32: two 16-byte stores
    static __device__ __forceinline__ void store8(void* base, int64_t off, const float (&y)[8]) {
        float* q = static_cast<float*>(base) + off;
        *reinterpret_cast<pq_f32x4*>(q) = pq_f32x4{y[0], y[1], y[2], y[3]};
        *reinterpret_cast<pq_f32x4*>(q + 4) = pq_f32x4{y[4], y[5], y[6], y[7]};
    }
};

// 8 fp32 values that do not change during the launch (a slice of the weight, of a shift or of a dot vector): two 16-byte loads
__device__ __forceinline__ void load_f32x8(const float* __restrict__ src, float (&w)[8]) {
    const pq_f32x4 a = *reinterpret_cast<const pq_f32x4*>(src), c = *reinterpret_cast<const pq_f32x4*>(src + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { w[i] = a[i]; w[4 + i] = c[i]; }
}

__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }

// the largest |y| of a chunk as a bit pattern (unsigned order = order of the magnitudes; any NaN wins)
__device__ __forceinline__ unsigned absmax8(const float (&y)[8]) {
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) m = umax(m, __float_as_uint(y[i]) & 0x7fffffffu);
    return m;
}

// z = y * inv clamped to +-448, the step in front of the e4m3 conversion (inv = 1 / descale, one IEEE division by the caller)
__device__ __forceinline__ void scale_clamp8(float (&y)[8], float inv) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float z = y[i] * inv;
        z = z > 448.f ? 448.f : z;                                 // a NaN fails both compares and stays
        y[i] = z < -448.f ? -448.f : z;
    }
}

}  // namespace
}  // namespace la
