// Internal: device helpers shared by the kernel units (wun_kernels, wun_elementwise, wun_bf16, wun_wgrad_bf16,
// wun_wgrad_win, wun_narrow, wun_track, wun_dataset).  Host units include wun_internal.h only.  gfx950 only.
#pragma once
#include "wun_internal.h"

namespace wun {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_cvoid_t;

// Workgroups are dealt round-robin to the 8 XCDs (each with its own L2).  Remap the hardware block
// id so that every XCD works on a CONTIGUOUS range of logical tiles: the tiles that share an input
// window (the N tiles of one time tile, neighbouring time tiles' halos; for the weight gradient all
// (row group, column group) tiles of one split) then hit the same L2 instead of fetching the window
// once per XCD.
__device__ __forceinline__ int xcd_contiguous_block(int bid, int grid) {
    const int per = grid >> 3, rem = grid & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    return xcd < rem ? xcd * (per + 1) + idx : rem * (per + 1) + (xcd - rem) * per + idx;
}

// ---- bf16 storage helpers: a tensor element type ET is float or bf16_t; values are converted to float on load and
// rounded to nearest-even (v_cvt_pk_bf16_f32) on store.  ET = float compiles to the plain accesses.
typedef unsigned short bf16_t;
__device__ __forceinline__ unsigned bf_pack2(float lo, float hi) {       // two fp32 -> packed bf16 pair (RNE)
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){lo, hi}, bf16x2));
}
__device__ __forceinline__ float bf_lo(unsigned v) { return __builtin_bit_cast(float, v << 16); }
__device__ __forceinline__ float bf_hi(unsigned v) { return __builtin_bit_cast(float, v & 0xFFFF0000u); }
template <typename ET> __device__ __forceinline__ float ld1(const ET* p, long long i);
template <> __device__ __forceinline__ float ld1<float>(const float* p, long long i) { return p[i]; }
template <> __device__ __forceinline__ float ld1<bf16_t>(const bf16_t* p, long long i) { return __builtin_bit_cast(float, (unsigned)p[i] << 16); }
template <typename ET> __device__ __forceinline__ void st1(ET* p, long long i, float v);
template <> __device__ __forceinline__ void st1<float>(float* p, long long i, float v) { p[i] = v; }
template <> __device__ __forceinline__ void st1<bf16_t>(bf16_t* p, long long i, float v) { p[i] = (bf16_t)(bf_pack2(v, 0.f) & 0xFFFFu); }
// four consecutive elements; p + i must be aligned to 4 elements (16 bytes fp32 / 8 bytes bf16)
template <typename ET> __device__ __forceinline__ f32x4 ld4(const ET* p, long long i);
template <> __device__ __forceinline__ f32x4 ld4<float>(const float* p, long long i) { return *reinterpret_cast<const f32x4*>(p + i); }
template <> __device__ __forceinline__ f32x4 ld4<bf16_t>(const bf16_t* p, long long i) {
    const u32x2 v = *reinterpret_cast<const u32x2*>(p + i);
    return (f32x4){bf_lo(v[0]), bf_hi(v[0]), bf_lo(v[1]), bf_hi(v[1])};
}
template <typename ET> __device__ __forceinline__ void st4(ET* p, long long i, f32x4 v);
template <> __device__ __forceinline__ void st4<float>(float* p, long long i, f32x4 v) { *reinterpret_cast<f32x4*>(p + i) = v; }
template <> __device__ __forceinline__ void st4<bf16_t>(bf16_t* p, long long i, f32x4 v) {
    *reinterpret_cast<u32x2*>(p + i) = (u32x2){bf_pack2(v[0], v[1]), bf_pack2(v[2], v[3])};
}

// ---- windows that start at any float of a plane (wun_track.hip, wun_dataset.hip) ----
// p[i .. i + 3] where p + i - M is 16-byte aligned (0 <= M < 4); floats outside [lo, hi) read as 0 and are not touched
template <int M>
__device__ __forceinline__ f32x4 ld4_window(const float* __restrict__ p, long long i, long long lo, long long hi) {
    constexpr int NG = M ? 2 : 1;
    float f[4 * NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        const long long a = i - M + 4 * j;
        if (a >= lo && a + 4 <= hi) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(p + a);
#pragma unroll
            for (int r = 0; r < 4; ++r) f[4 * j + r] = v[r];
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long k = a + r;
                const bool need = 4 * j + r >= M && 4 * j + r < M + 4;
                f[4 * j + r] = (need && k >= lo && k < hi) ? p[k] : 0.f;
            }
        }
    }
    return (f32x4){f[M], f[M + 1], f[M + 2], f[M + 3]};
}

__device__ __forceinline__ int granule_offset(const float* p, long long i) {
    return (int)(((long long)(reinterpret_cast<uintptr_t>(p) >> 2) + i) & 3);
}

// ---- gradient accumulation (wun_*backward_accumulate) ----
// Every final gradient float is written once, by one lane: its accumulating form reads the old value and adds the rounded fp32
// G the overwriting form would store -- one IEEE add, round to nearest even (torch's float32 a + b).  The pragma keeps hipcc
// from contracting the add with the product that produced G into an FMA (that would change the bits).
__device__ __forceinline__ float grad_acc_add(float old, float g) {
#pragma clang fp contract(off)
    return old + g;
}
template <bool ACC> __device__ __forceinline__ void grad_st(float* p, float g) {
    if constexpr (ACC) *p = grad_acc_add(*p, g);
    else *p = g;
}

// ---- conv output epilogue: what every conv kernel does with a finished value (after its own bias / LeakyReLU) ----
// mask (LeakyReLU derivative of the forward activation msk holds; msk may be null) -> accumulate (F_ACCUM: add what dst holds
// inside the range) -> store -> copies (`copy`: the launch's decimated copies of the value, or nothing).  ET is the element type
// of dst and msk.  The vector forms take W = 4 (a quad) or 8 (the phase-2 oct) consecutive outputs.

// F_ACCUM applies to the row positions lo <= pos < lo + len (ConvArgs.acc_lo / acc_len; len 0 is normalised to the whole row)
struct AccRange {
    int lo; unsigned len;
    __device__ __forceinline__ bool at(int pos) const { return (unsigned)(pos - lo) < len; }
    // does the vector at positions pos0 .. pos0 + W - 1 overlap the range: interval overlap, (unsigned)(pos0 - lo + W - 1) <
    // len + W - 1, written as "any lane inside" -- the same predicate, which compiles to fewer VGPRs in the conv epilogues
    template <int W> __device__ __forceinline__ bool touches(int pos0) const {
        bool t = false;
#pragma unroll
        for (int r = 0; r < W; ++r) t = t || at(pos0 + r);
        return t;
    }
};

__device__ __forceinline__ float conv_msk(float m) { return m > 0.f ? 1.f : 0.2f; }

// v[j][r] (j < W / 4) = output at dst[idx + 4j + r], accumulate position pos0 + 4j + r (W = 4: a quad, 8: the phase-2 oct;
// ostride 1, idx aligned to 4 elements); v is updated in place
template <int W, typename ET, typename Copy>
__device__ __forceinline__ void conv_out_vec(ET* dst, const ET* msk, long long idx, bool accum, AccRange rng, int pos0, f32x4* v,
                                             Copy&& copy) {
    if (msk != nullptr) {
#pragma unroll
        for (int j = 0; j < W / 4; ++j) {
            const f32x4 mk = ld4<ET>(msk, idx + 4 * j);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[j][r] *= conv_msk(mk[r]);
        }
    }
    if (accum && rng.touches<W>(pos0)) {
#pragma unroll
        for (int j = 0; j < W / 4; ++j) {
            const f32x4 old = ld4<ET>(dst, idx + 4 * j);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (rng.at(pos0 + 4 * j + r)) v[j][r] += old[r];
        }
    }
#pragma unroll
    for (int j = 0; j < W / 4; ++j) st4<ET>(dst, idx + 4 * j, v[j]);
    copy(v);
}
// the same for a quad whose mask and old values were loaded earlier (conv_out_side): a caller can issue those loads before
// it has the values
struct ConvSide { f32x4 mk, old; bool acc; };
template <typename ET>
__device__ __forceinline__ ConvSide conv_out_side(const ET* dst, const ET* msk, long long idx, bool accum, AccRange rng, int pos0) {
    ConvSide s = {{1.f, 1.f, 1.f, 1.f}, {0.f, 0.f, 0.f, 0.f}, accum && rng.touches<4>(pos0)};
    if (msk != nullptr) s.mk = ld4<ET>(msk, idx);
    if (s.acc) s.old = ld4<ET>(dst, idx);
    return s;
}
template <typename ET, typename Copy>
__device__ __forceinline__ void conv_out_vec(ET* dst, bool has_msk, long long idx, AccRange rng, int pos0, const ConvSide& s,
                                             f32x4* v, Copy&& copy) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (has_msk) v[0][r] *= conv_msk(s.mk[r]);
        if (s.acc && rng.at(pos0 + r)) v[0][r] += s.old[r];
    }
    st4<ET>(dst, idx, v[0]);
    copy(v);
}
// one output at dst[idx]; acc: F_ACCUM set and its position inside the range
template <typename ET, typename Copy>
__device__ __forceinline__ void conv_out1(ET* dst, const ET* msk, long long idx, bool acc, float v, Copy&& copy) {
    if (msk != nullptr) v *= conv_msk(ld1<ET>(msk, idx));
    if (acc) v += ld1<ET>(dst, idx);
    st1<ET>(dst, idx, v);
    copy(v);
}
// for the outputs without copies
struct NoCopy { template <typename T> __device__ __forceinline__ void operator()(const T&) const {} };

}  // namespace wun
