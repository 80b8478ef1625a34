// gfx950 (MI355X / CDNA4): recursive (IIR) filtering along time and the BS.1770-4 loudness meter built on it
// (include/wun.h: wun_sosfilt, wun_kweight_design, wun_loudness, wun_loudness_gain, wun_scale_by).
//
//   biquad cascade     y = sosfilt(sos, x) per channel from zero initial state, direct form I per section:
//                      y[t] = b0 x[t] + b1 x[t-1] + b2 x[t-2] - a1 y[t-1] - a2 y[t-2]      (float64, rounded once to float32)
//   loudness           K-weighting (two sections), mean squares over blocks of 0.4 s at a step of 0.1 s, absolute gate at
//                      -70 LUFS, relative gate 10 LU under the absolute-gated mean; the filtered signal is never written
//   R 128              the other figures of that meter (wun_true_peak, wun_loudness_r128): the true peak as the
//                      maximum of the resampler's oversampled output, never written; 3 s short-term blocks from the same walk
//                      of the recurrence; the loudness range, its two ranks selected by counting
//
// A recurrence is serial in time, so the SCHEDULE is part of the definition (the bits must not depend on the grid): time is
// cut into chunks of WUN_SOS_CHUNK frames, one lane per (chunk, channel).
//   pass 1   every chunk runs the cascade with the TRUE input history x[t0 - 1], x[t0 - 2] and zero recursive state
//            (y_s[t0 - 1] = y_s[t0 - 2] = 0 for every section s) and keeps its end state e_k: 2 nsec doubles
//   carry    the true start state v_k of every chunk: v_0 = 0, v_{k+1} = M v_k + e_k, where M = T^chunk is the homogeneous
//            transition of a whole chunk (T: one step with zero input; 2 nsec x 2 nsec, formed on the host in float64 by
//            repeated squaring).  Two levels: the first pass walks the 64 chunks of its workgroup (= carry group,
//            WUN_SOS_TILE) from zero and keeps the group's end; sos_group_kernel walks the group ends with M^tile into
//            the group starts; the last pass walks its group again from its true start.  The walks run in LDS by the
//            first wave of the workgroup, lane 16 c + r holding row r of M (sos_carry_walk).
//   pass 2   every chunk runs again from v_k and writes its outputs (the meter: accumulates squares instead)
// The state is (y_s[t - 1], y_s[t - 2]) per section in cascade order -- the companion basis of the recurrence as it is written.
// The last chunk may be short: its end state has no reader, so no power of T other than T^chunk is ever needed.
//
// Lanes own chunks, so a lane's samples lie chunk * C floats apart.  Global memory is touched only by cooperative copies
// between it and an LDS tile [chunk][32 frames][C] (32 C consecutive floats per chunk, >= 128 B); the row pitch 32 C + C
// puts the 32 lanes of a half wave on 32 different banks.  One workgroup = WUN_SOS_TILE chunks x C channels = 64 C lanes.
// Three launches per filter call: end states, group walk, outputs.
//
// Built WITHOUT the packed fp32 VALU instructions like wun_bsseval.hip (csrc/Makefile NO_PK_FP32).  Every
// argument check runs before any GPU work; nothing allocates or synchronises; no atomics; every sum has one order.
#include "wun_device.h"
#include "../../include/wun.h"

#include <cmath>
#include <cstring>
#include <string>

using namespace wun;
int fail(int code, const std::string& msg);      // wun_plan.hip: sets wun_last_error(), returns code

#define WUN_SOS_CHUNK 256            // frames per chunk: THE schedule constant (wun_sos_chunk)
#define WUN_SOS_TILE 64              // chunks per workgroup and per carry group (wun_sos_tile)
#define WUN_SOS_SUB 32               // frames of every chunk staged in LDS at a time
#define WUN_SOS_MAXSEC 8
#define WUN_SOS_MAXD (2 * WUN_SOS_MAXSEC)
#define WUN_LOUD_BLOCK 256           // lanes of the block-sum and gating kernels

namespace wun {      // the kernels carry the library's wun:: prefix in profiler output

struct SosCoef { double b0[WUN_SOS_MAXSEC], b1[WUN_SOS_MAXSEC], b2[WUN_SOS_MAXSEC], a1[WUN_SOS_MAXSEC], a2[WUN_SOS_MAXSEC]; int nsec; };
struct SosMat { double m[WUN_SOS_MAXD][WUN_SOS_MAXD]; };          // rows / columns beyond 2 nsec are not read

struct SosState { double x1, x2, y1[WUN_SOS_MAXSEC], y2[WUN_SOS_MAXSEC]; };

// one sample through the cascade: the one arithmetic order of the recurrence (products added left to right by FMA)
__device__ __forceinline__ double sos_step(const SosCoef& k, SosState& s, double xv) {
    double in = xv, in1 = s.x1, in2 = s.x2;
#pragma unroll
    for (int i = 0; i < WUN_SOS_MAXSEC; ++i) {
        if (i < k.nsec) {
            const double p1 = s.y1[i], p2 = s.y2[i];
            double y = k.b0[i] * in;
            y = fma(k.b1[i], in1, y);
            y = fma(k.b2[i], in2, y);
            y = fma(-k.a1[i], p1, y);
            y = fma(-k.a2[i], p2, y);
            s.y2[i] = p1; s.y1[i] = y;
            in = y; in1 = p1; in2 = p2;
        }
    }
    s.x2 = s.x1; s.x1 = xv;
    return in;
}

// the first block start (a multiple of step) and the first block end (Nb + a multiple of step) strictly inside (t0, t1),
// sorted; t1 where there is none.  step > WUN_SOS_CHUNK (sr >= 4000), so a chunk holds at most one of each: the cuts divide it
// into at most three pieces, and every piece lies wholly inside or wholly outside any block.
__host__ __device__ __forceinline__ void loud_cuts(long long t0, long long t1, long long Nb, long long step, long long& c1,
                                                   long long& c2) {
    long long bs = (t0 / step + 1) * step;
    long long be = t0 < Nb ? Nb : Nb + ((t0 - Nb) / step + 1) * step;
    if (bs > t1) bs = t1;
    if (be > t1) be = t1;
    c1 = bs < be ? bs : be;
    c2 = bs < be ? be : bs;
}

__device__ __forceinline__ double nan_max(double a, double b) { return (a != a || b != b) ? (a + b) : (a > b ? a : b); }

enum { SOS_END_STATE = 0, SOS_WRITE = 1, SOS_SQUARES = 2, SOS_SQUARES2 = 3 };    // SQUARES2: the 0.4 s and the 3 s pieces in one walk

struct SosChunkArgs {
    const float* x; float* y;        // [n, C]; y: SOS_WRITE only
    double* st;                      // [2 nsec][C][nchunks] end states e_k: SOS_END_STATE writes them, the other modes read them
    double* grp;                     // [2 nsec][C][ngroups]: SOS_END_STATE writes the group ends, the other modes read the group starts
    double* pieces;                  // SOS_SQUARES: [3][C][nchunks] sums of squares of the chunk's pieces
    double* peak;                    // SOS_SQUARES: [C][nchunks] max |x| of the chunk (NaN if it holds one)
    double* pieces3;                 // SOS_SQUARES2: [3][C][nchunks] the same squares cut at the 3 s blocks' starts and ends
    long long n, nchunks, ngroups, Nb, step, N3;
    SosCoef k;
    SosMat M;                        // the chunk transition
};

// The carry walk, by the first wave of a workgroup: v <- M v + e_k over the `count` items of es[k][CH][16] (LDS) in ascending
// k.  Lane 16 c + r holds row r of M and component r of channel c's state; a step fetches the other components from the lanes
// beside it and adds row r's products in ascending column order by FMA, starting from e_k[r] -- the one order of the carry.
// REPLACE: every item is replaced by the state in front of it.  All 64 lanes run it (the exchanges need them); lanes with
// r >= D or c >= CH compute nothing that is kept.  Returns the state behind the last item.
template <int CH, bool REPLACE>
__device__ __forceinline__ double sos_carry_walk(const SosMat& Ms, int D, double v, double* es, int count) {
    const int lane = threadIdx.x & 63, r = lane & 15, c = lane >> 4, base = lane & 48;
    const bool ok = r < D && c < CH;
    double mrow[WUN_SOS_MAXD];
#pragma unroll
    for (int q = 0; q < WUN_SOS_MAXD; ++q) mrow[q] = Ms.m[r][q];
    double* at = es + (c < CH ? c : 0) * WUN_SOS_MAXD + r;
    for (int k = 0; k < count; ++k, at += CH * WUN_SOS_MAXD) {
        double acc = *at;
        if (REPLACE && ok) *at = v;
#pragma unroll
        for (int q = 0; q < WUN_SOS_MAXD; ++q)
            if (q < D) acc = fma(mrow[q], __shfl(v, base + q), acc);
        v = acc;
    }
    return v;
}

// grid.x = tile (= carry group) of WUN_SOS_TILE chunks; block = WUN_SOS_TILE * CH lanes, lane = chunk * CH + channel.
// SOS_END_STATE: the chunks from zero recursive state; their end states go to st and, walked from zero, the group's end to grp.
// SOS_WRITE / SOS_SQUARES: the group is walked again from its true start (grp, after sos_group_kernel), then the chunks run
// from their true states.
template <int CH, int MODE>
__global__ __launch_bounds__(WUN_SOS_TILE * CH) void sos_chunk_kernel(SosChunkArgs p) {
    constexpr int PITCH = WUN_SOS_SUB * CH + CH;
    constexpr int NT = WUN_SOS_TILE * CH;
    __shared__ float tile[WUN_SOS_TILE * PITCH];
    __shared__ double es[WUN_SOS_TILE * CH * WUN_SOS_MAXD];  // [chunk][CH][16]: end states / start states of the tile's chunks
    __shared__ SosMat Ms;
    const int tid = threadIdx.x;
    const int lc = tid / CH, c = tid % CH;
    const long long T0 = (long long)blockIdx.x * WUN_SOS_TILE * WUN_SOS_CHUNK;       // first frame of the tile
    const long long kc = (long long)blockIdx.x * WUN_SOS_TILE + lc;                  // this lane's chunk
    const long long t0 = kc * WUN_SOS_CHUNK;
    const bool live = kc < p.nchunks;                                                // t0 < n
    const int D = 2 * p.k.nsec;
    const long long left = p.nchunks - (long long)blockIdx.x * WUN_SOS_TILE;
    const int count = left < WUN_SOS_TILE ? (int)left : WUN_SOS_TILE;                // chunks of this tile
    const int wr = tid & 15, wc = (tid >> 4) & 3;                                    // the walk's row and channel (first wave)
    const bool walk_ok = tid < 64 && wr < D && wc < CH;

    for (int q = tid; q < WUN_SOS_MAXD * WUN_SOS_MAXD; q += NT) Ms.m[q / WUN_SOS_MAXD][q % WUN_SOS_MAXD] = p.M.m[q / WUN_SOS_MAXD][q % WUN_SOS_MAXD];

    SosState s;
    s.x1 = (live && t0 >= 1) ? (double)p.x[(t0 - 1) * CH + c] : 0.0;                 // the true input history
    s.x2 = (live && t0 >= 2) ? (double)p.x[(t0 - 2) * CH + c] : 0.0;
#pragma unroll
    for (int i = 0; i < WUN_SOS_MAXSEC; ++i) { s.y1[i] = 0.0; s.y2[i] = 0.0; }
    if (MODE != SOS_END_STATE) {
        if (live) {
#pragma unroll
            for (int r = 0; r < WUN_SOS_MAXD; ++r)
                if (r < D) es[(lc * CH + c) * WUN_SOS_MAXD + r] = p.st[((long long)r * CH + c) * p.nchunks + kc];
        }
        __syncthreads();
        if (tid < 64) {
            const double v0 = walk_ok ? p.grp[((long long)wr * CH + wc) * p.ngroups + blockIdx.x] : 0.0;
            sos_carry_walk<CH, true>(Ms, D, v0, es, count);
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int i = 0; i < WUN_SOS_MAXSEC; ++i)
                if (i < p.k.nsec) {
                    s.y1[i] = es[(lc * CH + c) * WUN_SOS_MAXD + 2 * i];
                    s.y2[i] = es[(lc * CH + c) * WUN_SOS_MAXD + 2 * i + 1];
                }
        }
    }
    constexpr bool SQ = MODE == SOS_SQUARES || MODE == SOS_SQUARES2;
    long long c1 = 0, c2 = 0, d1 = 0, d2 = 0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, pk = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (SQ) {
        const long long t1 = t0 + WUN_SOS_CHUNK < p.n ? t0 + WUN_SOS_CHUNK : p.n;
        loud_cuts(t0, t1, p.Nb, p.step, c1, c2);
        if (MODE == SOS_SQUARES2) loud_cuts(t0, t1, p.N3, p.step, d1, d2);
    }

    for (int sub = 0; sub < WUN_SOS_CHUNK / WUN_SOS_SUB; ++sub) {
        __syncthreads();                                     // the previous sub-tile is consumed
        for (int e = tid; e < WUN_SOS_TILE * WUN_SOS_SUB * CH; e += NT) {
            const int ch = e / (WUN_SOS_SUB * CH), r = e % (WUN_SOS_SUB * CH);
            const long long f = T0 + (long long)ch * WUN_SOS_CHUNK + sub * WUN_SOS_SUB + r / CH;
            tile[ch * PITCH + r] = f < p.n ? p.x[f * CH + r % CH] : 0.f;
        }
        __syncthreads();
        if (live) {
            float* row = tile + lc * PITCH + c;
            const long long ts = t0 + sub * WUN_SOS_SUB;
            for (int j = 0; j < WUN_SOS_SUB; ++j) {
                const long long t = ts + j;
                if (t >= p.n) break;
                const float xf = row[j * CH];
                const double yv = sos_step(p.k, s, (double)xf);
                if (MODE == SOS_WRITE) row[j * CH] = (float)yv;
                if (SQ) {
                    if (t < c1) a0 = fma(yv, yv, a0);
                    else if (t < c2) a1 = fma(yv, yv, a1);
                    else a2 = fma(yv, yv, a2);
                    pk = nan_max(pk, fabs((double)xf));
                }
                if (MODE == SOS_SQUARES2) {                  // the same sample into the 3 s pieces: own sums, own cuts
                    if (t < d1) s0 = fma(yv, yv, s0);
                    else if (t < d2) s1 = fma(yv, yv, s1);
                    else s2 = fma(yv, yv, s2);
                }
            }
        }
        if (MODE == SOS_WRITE) {
            __syncthreads();
            for (int e = tid; e < WUN_SOS_TILE * WUN_SOS_SUB * CH; e += NT) {
                const int ch = e / (WUN_SOS_SUB * CH), r = e % (WUN_SOS_SUB * CH);
                const long long f = T0 + (long long)ch * WUN_SOS_CHUNK + sub * WUN_SOS_SUB + r / CH;
                if (f < p.n) p.y[f * CH + r % CH] = tile[ch * PITCH + r];
            }
        }
    }
    if (MODE == SOS_END_STATE) {
        if (live) {
#pragma unroll
            for (int i = 0; i < WUN_SOS_MAXSEC; ++i) {
                if (i < p.k.nsec) {
                    es[(lc * CH + c) * WUN_SOS_MAXD + 2 * i] = s.y1[i];
                    es[(lc * CH + c) * WUN_SOS_MAXD + 2 * i + 1] = s.y2[i];
                    p.st[((long long)(2 * i) * CH + c) * p.nchunks + kc] = s.y1[i];
                    p.st[((long long)(2 * i + 1) * CH + c) * p.nchunks + kc] = s.y2[i];
                }
            }
        }
        __syncthreads();
        if (tid < 64) {
            const double v = sos_carry_walk<CH, false>(Ms, D, 0.0, es, count);
            if (walk_ok) p.grp[((long long)wr * CH + wc) * p.ngroups + blockIdx.x] = v;
        }
    }
    if (SQ && live) {
        p.pieces[((long long)0 * CH + c) * p.nchunks + kc] = a0;
        p.pieces[((long long)1 * CH + c) * p.nchunks + kc] = a1;
        p.pieces[((long long)2 * CH + c) * p.nchunks + kc] = a2;
        p.peak[(long long)c * p.nchunks + kc] = pk;
    }
    if (MODE == SOS_SQUARES2 && live) {
        p.pieces3[((long long)0 * CH + c) * p.nchunks + kc] = s0;
        p.pieces3[((long long)1 * CH + c) * p.nchunks + kc] = s1;
        p.pieces3[((long long)2 * CH + c) * p.nchunks + kc] = s2;
    }
}

#define WUN_SOS_GROUP_BATCH 128      // group ends staged in LDS at a time by the second level of the carry

// The second level, ONE wave: the group ends grp[D][CH][ngroups] are walked from zero with M^tile and replaced by the group
// starts.  The series passes through LDS in batches (coalesced copies in and out), so a step costs an LDS exchange, not a
// round trip to memory.
template <int CH>
__global__ __launch_bounds__(64) void sos_group_kernel(SosMat MG, int D, double* grp, long long ngroups) {
    __shared__ double es[WUN_SOS_GROUP_BATCH * CH * WUN_SOS_MAXD];
    __shared__ SosMat Ms;
    const int tid = threadIdx.x;
    for (int q = tid; q < WUN_SOS_MAXD * WUN_SOS_MAXD; q += 64) Ms.m[q / WUN_SOS_MAXD][q % WUN_SOS_MAXD] = MG.m[q / WUN_SOS_MAXD][q % WUN_SOS_MAXD];
    double v = 0.0;
    for (long long j0 = 0; j0 < ngroups; j0 += WUN_SOS_GROUP_BATCH) {
        const int cnt = ngroups - j0 < WUN_SOS_GROUP_BATCH ? (int)(ngroups - j0) : WUN_SOS_GROUP_BATCH;
        __syncthreads();
        for (int i = tid; i < D * CH * cnt; i += 64) {
            const int rc = i / cnt, j = i % cnt;             // rc = r * CH + c
            es[(j * CH + rc % CH) * WUN_SOS_MAXD + rc / CH] = grp[(long long)rc * ngroups + j0 + j];
        }
        __syncthreads();
        v = sos_carry_walk<CH, true>(Ms, D, v, es, cnt);
        __syncthreads();
        for (int i = tid; i < D * CH * cnt; i += 64) {
            const int rc = i / cnt, j = i % cnt;
            grp[(long long)rc * ngroups + j0 + j] = es[(j * CH + rc % CH) * WUN_SOS_MAXD + rc / CH];
        }
    }
}

// z_j of block j = sum over channels (ascending) of [sum of the block's pieces in ascending (chunk, piece) order] / Nb
__device__ __forceinline__ void loud_block_body(const double* __restrict__ pieces, double* __restrict__ z, long long n,
                                                long long nchunks, long long nb, long long Nb, long long step, int C,
                                                long long j) {
    if (j >= nb) return;
    const long long s = j * step, e = s + Nb;
    double zj = 0.0;
    for (int c = 0; c < C; ++c) {
        double acc = 0.0;
        for (long long k = s / WUN_SOS_CHUNK; k <= (e - 1) / WUN_SOS_CHUNK; ++k) {
            const long long t0 = k * WUN_SOS_CHUNK, t1 = t0 + WUN_SOS_CHUNK < n ? t0 + WUN_SOS_CHUNK : n;
            long long c1, c2;
            loud_cuts(t0, t1, Nb, step, c1, c2);
            const long long lo[3] = {t0, c1, c2}, hi[3] = {c1, c2, t1};
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (lo[q] < hi[q] && lo[q] >= s && hi[q] <= e) acc += pieces[((long long)q * C + c) * nchunks + k];
        }
        zj += acc / (double)Nb;
    }
    z[j] = zj;
}

__global__ __launch_bounds__(WUN_LOUD_BLOCK) void loud_block_kernel(const double* __restrict__ pieces, double* __restrict__ z,
                                                                    long long n, long long nchunks, long long nb, long long Nb,
                                                                    long long step, int C) {
    loud_block_body(pieces, z, n, nchunks, nb, Nb, step, C, (long long)blockIdx.x * WUN_LOUD_BLOCK + threadIdx.x);
}

// both window lengths in one launch: the first g workgroups sum the 0.4 s blocks, the others the 3 s blocks, one lane per block
__global__ __launch_bounds__(WUN_LOUD_BLOCK) void loud_block2_kernel(const double* __restrict__ pieces, double* __restrict__ z,
                                                                     long long nb, long long Nb, const double* __restrict__ pieces3,
                                                                     double* __restrict__ z3, long long nb3, long long N3, long long n,
                                                                     long long nchunks, long long step, int C, unsigned g) {
    if (blockIdx.x < g) loud_block_body(pieces, z, n, nchunks, nb, Nb, step, C, (long long)blockIdx.x * WUN_LOUD_BLOCK + threadIdx.x);
    else loud_block_body(pieces3, z3, n, nchunks, nb3, N3, step, C, (long long)(blockIdx.x - g) * WUN_LOUD_BLOCK + threadIdx.x);
}

// the fixed tree over the lanes of the one gating workgroup; every lane gets the total
__device__ __forceinline__ double loud_tree(double* red, double v, int tid, bool is_max) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = WUN_LOUD_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = is_max ? nan_max(red[tid], red[tid + s]) : red[tid] + red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ double loud_lufs(double z) { return -0.691 + 10.0 * log10(z); }

// ONE workgroup: momentary values, both gates, the result and the peak.  Lane i adds the blocks i, i + 256, ... in ascending
// order, then the tree adds the lanes.  A NaN block (a NaN or an infinity in x) makes L NaN: the gates alone would drop it.
// MOM: also the largest momentary value (-inf with no block, NaN with a NaN block) into *mom
template <bool MOM>
__device__ __forceinline__ void loud_gate_body(double* red, const double* __restrict__ z, long long nb,
                                               const double* __restrict__ peak, long long npeak, double* __restrict__ meter,
                                               double* __restrict__ blocks, double* __restrict__ mom) {
    const int tid = threadIdx.x;
    double sum = 0.0, cnt = 0.0, bad = 0.0, top = -HUGE_VAL;
    for (long long j = tid; j < nb; j += WUN_LOUD_BLOCK) {
        const double l = loud_lufs(z[j]);
        if (blocks) blocks[j] = l;
        if (l != l) bad = 1.0;
        if (MOM) top = nan_max(top, l);
        if (l > -70.0) { sum += z[j]; cnt += 1.0; }
    }
    if (MOM) {
        top = loud_tree(red, top, tid, true);
        if (tid == 0) *mom = top;
    }
    sum = loud_tree(red, sum, tid, false);
    cnt = loud_tree(red, cnt, tid, false);
    bad = loud_tree(red, bad, tid, false);
    const double gate = cnt > 0.0 ? loud_lufs(sum / cnt) - 10.0 : 0.0;
    double sum2 = 0.0, cnt2 = 0.0;
    if (cnt > 0.0) {
        for (long long j = tid; j < nb; j += WUN_LOUD_BLOCK) {
            const double l = loud_lufs(z[j]);
            if (l > -70.0 && l > gate) { sum2 += z[j]; cnt2 += 1.0; }
        }
    }
    sum2 = loud_tree(red, sum2, tid, false);
    cnt2 = loud_tree(red, cnt2, tid, false);
    double pk = 0.0;
#pragma unroll 4
    for (long long i = tid; i < npeak; i += WUN_LOUD_BLOCK) pk = nan_max(pk, peak[i]);
    pk = loud_tree(red, pk, tid, true);
    if (tid == 0) {
        double L = cnt2 > 0.0 ? loud_lufs(sum2 / cnt2) : -HUGE_VAL;
        if (bad > 0.0) L = nan("");
        meter[0] = L; meter[1] = cnt2; meter[2] = (double)nb; meter[3] = pk;
    }
}

__global__ __launch_bounds__(WUN_LOUD_BLOCK) void loud_gate_kernel(const double* __restrict__ z, long long nb,
                                                                   const double* __restrict__ peak, long long npeak,
                                                                   double* __restrict__ meter, double* __restrict__ blocks) {
    __shared__ double red[WUN_LOUD_BLOCK];
    loud_gate_body<false>(red, z, nb, peak, npeak, meter, blocks, nullptr);
}

// ---- EBU R 128: short-term gating, loudness range, true peak ----------------------------------------------
#define WUN_TP_TILE 1024             // input frames per workgroup of the peak kernel
#define WUN_TP_BLOCK 256
#define WUN_TP_K 21                  // taps per phase of wun_resample_design(L, 1) for every L >= 2: ceil((20 L + 1) / L)
#define WUN_TP_MAXL 32
#define WUN_LRA_TILE 1024            // keys staged in LDS at a time by the selection kernel
#define WUN_LRA_MAX_BLOCKS (1 << 20) // short-term blocks the quadratic selection accepts (29 hours)

// st[0] = m, the short-term blocks past both gates; st[1] > 0: a NaN block; st[2] = the largest s_j.  key[j] = s_j for a
// block that passes, +inf otherwise: what lra_select_kernel orders.  The gating sums as in loud_gate_body.
__device__ __forceinline__ void st_gate_body(double* red, const double* __restrict__ z3, long long nb3, double* __restrict__ key,
                                             double* __restrict__ short_term, double* __restrict__ st) {
    const int tid = threadIdx.x;
    double sum = 0.0, cnt = 0.0, bad = 0.0, top = -HUGE_VAL;
    for (long long j = tid; j < nb3; j += WUN_LOUD_BLOCK) {
        const double s = loud_lufs(z3[j]);
        if (short_term) short_term[j] = s;
        if (s != s) bad = 1.0;
        top = nan_max(top, s);
        if (s > -70.0) { sum += z3[j]; cnt += 1.0; }
    }
    top = loud_tree(red, top, tid, true);
    sum = loud_tree(red, sum, tid, false);
    cnt = loud_tree(red, cnt, tid, false);
    bad = loud_tree(red, bad, tid, false);
    const double gate = cnt > 0.0 ? loud_lufs(sum / cnt) - 20.0 : 0.0;
    double m = 0.0;
    for (long long j = tid; j < nb3; j += WUN_LOUD_BLOCK) {
        const double s = loud_lufs(z3[j]);
        const bool keep = cnt > 0.0 && s > -70.0 && s > gate;
        key[j] = keep ? s : HUGE_VAL;
        if (keep) m += 1.0;
    }
    m = loud_tree(red, m, tid, false);
    if (tid == 0) { st[0] = m; st[1] = bad; st[2] = top; }
}

// workgroup 0: the meter of wun_loudness (+ the largest momentary value); workgroup 1: the short-term gating
__global__ __launch_bounds__(WUN_LOUD_BLOCK) void r128_gate_kernel(const double* __restrict__ z, long long nb,
                                                                   const double* __restrict__ peak, long long npeak,
                                                                   double* __restrict__ meter, double* __restrict__ mom,
                                                                   const double* __restrict__ z3, long long nb3,
                                                                   double* __restrict__ key, double* __restrict__ short_term,
                                                                   double* __restrict__ st) {
    __shared__ double red[WUN_LOUD_BLOCK];
    if (blockIdx.x == 0) loud_gate_body<true>(red, z, nb, peak, npeak, meter, nullptr, mom);
    else st_gate_body(red, z3, nb3, key, short_term, st);
}

// The two ranks of the loudness range, without sorting: lane j counts the keys that order before its own by (value, index);
// the counts of the m blocks that pass are a permutation of 0 .. m - 1, so exactly one lane holds each wanted rank and writes
// its value.  No atomics, no host value; nb3^2 comparisons over the grid, the keys passing through LDS.
__global__ __launch_bounds__(WUN_LOUD_BLOCK) void lra_select_kernel(const double* __restrict__ key, long long nb3,
                                                                    const double* __restrict__ st, double* __restrict__ sel) {
    __shared__ double tile[WUN_LRA_TILE];
    const int tid = threadIdx.x;
    const long long j = (long long)blockIdx.x * WUN_LOUD_BLOCK + tid;
    const double kj = j < nb3 ? key[j] : HUGE_VAL;
    long long before = 0;
    for (long long i0 = 0; i0 < nb3; i0 += WUN_LRA_TILE) {
        const int cnt = nb3 - i0 < WUN_LRA_TILE ? (int)(nb3 - i0) : WUN_LRA_TILE;
        __syncthreads();
        for (int i = tid; i < cnt; i += WUN_LOUD_BLOCK) tile[i] = key[i0 + i];
        __syncthreads();
        for (int i = 0; i < cnt; ++i) {
            const double ki = tile[i];
            before += (ki < kj || (ki == kj && i0 + i < j)) ? 1 : 0;
        }
    }
    if (kj < HUGE_VAL) {
        const long long m = (long long)st[0];
        if (before == ((m - 1) * 10 + 50) / 100) sel[0] = kj;
        if (before == ((m - 1) * 95 + 50) / 100) sel[1] = kj;
    }
}

struct PeakArgs { const float* x; const float* taps; double* part; long long n; int L; };

// max |r| of the signal oversampled by L, r never written: r[t] is wun_resample's output for up = L, down = 1 bit for bit --
// u = t + 10 L, q = u / L = t / L + 10, p = u % L = t % L, acc = fmaf(taps[p K + k], v[q - k], acc) for k ascending, +0
// outside the input.  A workgroup stages WUN_TP_TILE frames with their 10-frame halo on both sides and the table in LDS; a
// lane takes a frame f, keeps the 21 samples v[f + 10 - k] in registers and walks the L phases of that frame.  A maximum
// does not depend on the order: wave shuffles, then LDS, one partial per workgroup and channel (NaN when the channel holds a
// NaN SAMPLE in the tile: the comparison drops the NaNs an infinity makes of r).  L == 1: r = x.
template <int CL>
__global__ __launch_bounds__(WUN_TP_BLOCK) void true_peak_kernel(PeakArgs a) {
    constexpr int W = WUN_TP_TILE + WUN_TP_K - 1, H = (WUN_TP_K - 1) / 2;
    __shared__ __attribute__((aligned(16))) float win[W * CL];
    __shared__ float tab[WUN_TP_MAXL * WUN_TP_K];
    __shared__ float red[(WUN_TP_BLOCK / 64) * CL];
    __shared__ int redbad[(WUN_TP_BLOCK / 64) * CL];
    const int tid = threadIdx.x;
    const long long F0 = (long long)blockIdx.x * WUN_TP_TILE;
    for (int i = tid; i < W * CL; i += WUN_TP_BLOCK) {
        const long long m = F0 - H + i / CL;
        win[i] = (m >= 0 && m < a.n) ? a.x[m * CL + i % CL] : 0.f;
    }
    if (a.L > 1)
        for (int i = tid; i < a.L * WUN_TP_K; i += WUN_TP_BLOCK) tab[i] = a.taps[i];
    __syncthreads();

    float mx[CL];
    bool bad[CL];
#pragma unroll
    for (int c = 0; c < CL; ++c) { mx[c] = 0.f; bad[c] = false; }
    for (int fl = tid; fl < WUN_TP_TILE && F0 + fl < a.n; fl += WUN_TP_BLOCK) {
        float v[WUN_TP_K][CL];
#pragma unroll
        for (int k = 0; k < WUN_TP_K; ++k) {
            const int j = fl + WUN_TP_K - 1 - k;                 // window index of v[q - k]
            if (CL == 2) {
                const f32x2 w = *reinterpret_cast<const f32x2*>(win + 2 * j);
                v[k][0] = w[0]; v[k][CL - 1] = w[1];
            } else {
                v[k][0] = win[j];
            }
        }
#pragma unroll
        for (int c = 0; c < CL; ++c)
            if (v[H][c] != v[H][c]) bad[c] = true;               // v[H] is the frame's own sample
        if (a.L == 1) {
#pragma unroll
            for (int c = 0; c < CL; ++c) {
                const float r = fabsf(v[H][c]);
                if (r > mx[c]) mx[c] = r;
            }
        } else {
            for (int p = 0; p < a.L; ++p) {
                const float* row = tab + p * WUN_TP_K;
                float acc[CL];
#pragma unroll
                for (int c = 0; c < CL; ++c) acc[c] = 0.f;
#pragma unroll
                for (int k = 0; k < WUN_TP_K; ++k) {             // k ascending: the resampler's one accumulation order
                    const float h = row[k];
#pragma unroll
                    for (int c = 0; c < CL; ++c) acc[c] = fmaf(h, v[k][c], acc[c]);
                }
#pragma unroll
                for (int c = 0; c < CL; ++c) {
                    const float r = fabsf(acc[c]);
                    if (r > mx[c]) mx[c] = r;
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CL; ++c) {
        for (int off = 32; off > 0; off >>= 1) {
            const float o = __shfl_xor(mx[c], off);
            if (o > mx[c]) mx[c] = o;
        }
        const int anybad = __any(bad[c] ? 1 : 0);
        if ((tid & 63) == 0) { red[(tid >> 6) * CL + c] = mx[c]; redbad[(tid >> 6) * CL + c] = anybad; }
    }
    __syncthreads();
    if (tid < CL) {
        float m = red[tid];
        int b = redbad[tid];
        for (int w = 1; w < WUN_TP_BLOCK / 64; ++w) {
            const float o = red[w * CL + tid];
            if (o > m) m = o;
            b |= redbad[w * CL + tid];
        }
        a.part[(long long)blockIdx.x * CL + tid] = b ? nan("") : (double)m;
    }
}

// the partials [nwg][C] of true_peak_kernel into per-channel maxima (tid 0: per_channel[c], when given) and the overall one
__device__ __forceinline__ double tp_combine(double* red, const double* __restrict__ part, long long nwg, int C,
                                             double* __restrict__ per_channel) {
    const int tid = threadIdx.x;
    double all = 0.0;
    for (int c = 0; c < C; ++c) {
        double pk = 0.0;
        for (long long i = tid; i < nwg; i += WUN_LOUD_BLOCK) pk = nan_max(pk, part[i * C + c]);
        pk = loud_tree(red, pk, tid, true);
        if (per_channel && tid == 0) per_channel[c] = pk;
        all = nan_max(all, pk);
    }
    return all;
}

__global__ __launch_bounds__(WUN_LOUD_BLOCK) void true_peak_finish_kernel(const double* __restrict__ part, long long nwg, int C,
                                                                         double* __restrict__ out) {
    __shared__ double red[WUN_LOUD_BLOCK];
    const double all = tp_combine(red, part, nwg, C, out + 1);
    if (threadIdx.x == 0) out[0] = all;
}

// ONE workgroup: the true peak from its partials, the range from the two selected values, the rest copied
__global__ __launch_bounds__(WUN_LOUD_BLOCK) void r128_report_kernel(const double* __restrict__ meter, const double* __restrict__ mom,
                                                                    const double* __restrict__ st, const double* __restrict__ sel,
                                                                    const double* __restrict__ part, long long nwg, int C,
                                                                    double* __restrict__ report) {
    __shared__ double red[WUN_LOUD_BLOCK];
    const double tp = tp_combine(red, part, nwg, C, nullptr);
    if (threadIdx.x == 0) {
        const double m = st[0];
        double lra = 0.0;
        if (m > 0.0) lra = sel[1] - sel[0];
        if (st[1] > 0.0) lra = nan("");
        report[0] = meter[0]; report[1] = lra; report[2] = mom[0]; report[3] = st[2];
        report[4] = tp; report[5] = meter[3]; report[6] = meter[1]; report[7] = m;
    }
}

__global__ void loud_gain_kernel(const double* __restrict__ meter, double target, double max_gain_db, double peak_limit,
                                 float* __restrict__ gain) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double L = meter[0], pk = meter[3];
    double g = 1.0;
    if (L == L && fabs(L) != HUGE_VAL) {
        g = pow(10.0, (target - L) / 20.0);
        const double cap = pow(10.0, max_gain_db / 20.0);
        if (g > cap) g = cap;
        if (peak_limit > 0.0 && pk > 0.0 && g * pk > peak_limit) g = peak_limit / pk;
    }
    const float gf = (float)g;
    gain[0] = gf;
    gain[1] = (float)(1.0 / (double)gf);
}

__global__ __launch_bounds__(256) void scale_by_kernel(float* __restrict__ x, long long count, const float* __restrict__ gain) {
    const float g = *gain;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += stride) x[i] *= g;
}

}  // namespace wun

namespace {

struct SosPlan { SosCoef k; SosMat M, MG; int D; };

void mat_square(double (*m)[WUN_SOS_MAXD], int D) {
    double r[WUN_SOS_MAXD][WUN_SOS_MAXD];
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) {
            double a = 0.0;
            for (int q = 0; q < D; ++q) a += m[i][q] * m[q][j];
            r[i][j] = a;
        }
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) m[i][j] = r[i][j];
}

// the coefficients in the kernels' layout and the chunk / group transitions M = T^chunk, MG = M^tile (repeated squaring:
// chunk and tile are powers of two).  T is one step of the cascade with zero input on the state (y_s[t-1], y_s[t-2])_s.
int sos_plan(const char* who, const double* sos, int32_t nsec, SosPlan* p) {
    if (!sos) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    if (nsec < 1 || nsec > WUN_SOS_MAXSEC) return fail(WUN_ERR_INVALID, std::string(who) + ": nsec outside 1..8");
    std::memset(p, 0, sizeof(*p));
    for (int s = 0; s < nsec; ++s) {
        const double* c = sos + 6 * s;
        for (int i = 0; i < 6; ++i)
            if (!std::isfinite(c[i])) return fail(WUN_ERR_INVALID, std::string(who) + ": a coefficient is not finite");
        if (c[3] != 1.0) return fail(WUN_ERR_INVALID, std::string(who) + ": a0 must be 1 (normalise the section)");
        p->k.b0[s] = c[0]; p->k.b1[s] = c[1]; p->k.b2[s] = c[2]; p->k.a1[s] = c[4]; p->k.a2[s] = c[5];
    }
    p->k.nsec = nsec;
    const int D = p->D = 2 * nsec;
    // column q of T: the state after one zero-input step from the unit state e_q
    for (int q = 0; q < D; ++q) {
        double y1[WUN_SOS_MAXSEC] = {0}, y2[WUN_SOS_MAXSEC] = {0};
        (q % 2 ? y2 : y1)[q / 2] = 1.0;
        double in = 0.0, in1 = 0.0, in2 = 0.0;
        for (int s = 0; s < nsec; ++s) {
            const double p1 = y1[s], p2 = y2[s];
            const double y = p->k.b0[s] * in + p->k.b1[s] * in1 + p->k.b2[s] * in2 - p->k.a1[s] * p1 - p->k.a2[s] * p2;
            p->M.m[2 * s][q] = y; p->M.m[2 * s + 1][q] = p1;
            in = y; in1 = p1; in2 = p2;
        }
    }
    for (int b = 1; b < WUN_SOS_CHUNK; b <<= 1) mat_square(p->M.m, D);
    p->MG = p->M;
    for (int b = 1; b < WUN_SOS_TILE; b <<= 1) mat_square(p->MG.m, D);
    return WUN_OK;
}

int64_t n_chunks(int64_t n) { return (n + WUN_SOS_CHUNK - 1) / WUN_SOS_CHUNK; }
int64_t n_groups(int64_t n) { return (n_chunks(n) + WUN_SOS_TILE - 1) / WUN_SOS_TILE; }
int64_t state_doubles(int64_t n, int32_t C, int32_t nsec) { return (int64_t)2 * nsec * C * (n_chunks(n) + n_groups(n)); }

int check_audio(const char* who, int64_t n, int32_t C) {
    if (n < 1) return fail(WUN_ERR_INVALID, std::string(who) + ": n < 1");
    if (C != 1 && C != 2) return fail(WUN_ERR_INVALID, std::string(who) + ": C must be 1 or 2");
    if (n > ((int64_t)1 << 40)) return fail(WUN_ERR_UNSUPPORTED, std::string(who) + ": more than 2^40 frames");
    return WUN_OK;
}

int check_scratch(const char* who, const double* scratch) {
    if (!scratch) return fail(WUN_ERR_INVALID, std::string(who) + ": null argument");
    if (reinterpret_cast<uintptr_t>(scratch) % 8) return fail(WUN_ERR_INVALID, std::string(who) + ": scratch is not 8-byte aligned");
    return WUN_OK;
}

void block_geometry(int32_t sr, int64_t n, int64_t* Nb, int64_t* step, int64_t* nb) {
    *Nb = ((int64_t)4 * sr + 5) / 10;                      // round(0.4 sr) and round(0.1 sr), halves up, in integers
    *step = ((int64_t)sr + 5) / 10;
    *nb = n >= *Nb ? (n - *Nb) / *step + 1 : 0;
}

// the three launches of the schedule; `a` carries the entry's own pointers, MODE is its last pass
template <int CH, int MODE>
void launch_schedule(const SosPlan& p, SosChunkArgs a, int64_t n, double* st, hipStream_t s) {
    const long long nch = n_chunks(n), ng = n_groups(n);
    a.st = st; a.grp = st + (long long)p.D * CH * nch; a.n = n; a.nchunks = nch; a.ngroups = ng; a.k = p.k; a.M = p.M;
    const dim3 grid((unsigned)ng), blk(WUN_SOS_TILE * CH);
    hipLaunchKernelGGL((sos_chunk_kernel<CH, SOS_END_STATE>), grid, blk, 0, s, a);
    hipLaunchKernelGGL(sos_group_kernel<CH>, dim3(1), dim3(64), 0, s, p.MG, p.D, a.grp, ng);
    hipLaunchKernelGGL((sos_chunk_kernel<CH, MODE>), grid, blk, 0, s, a);
}

}  // namespace

extern "C" int32_t wun_sos_chunk(void) { return WUN_SOS_CHUNK; }
extern "C" int32_t wun_sos_tile(void) { return WUN_SOS_TILE; }

extern "C" int64_t wun_sosfilt_scratch_doubles(int64_t n, int32_t C, int32_t nsec) {
    int rc;
    if ((rc = check_audio("wun_sosfilt_scratch_doubles", n, C))) return rc;
    if (nsec < 1 || nsec > WUN_SOS_MAXSEC) return fail(WUN_ERR_INVALID, "wun_sosfilt_scratch_doubles: nsec outside 1..8");
    return state_doubles(n, C, nsec);
}

extern "C" int wun_sosfilt(const float* x, int64_t n, int32_t C, const double* sos, int32_t nsec, float* y, double* scratch,
                           void* stream) {
    if (!x || !y) return fail(WUN_ERR_INVALID, "wun_sosfilt: null argument");
    int rc;
    if ((rc = check_scratch("wun_sosfilt", scratch))) return rc;
    if ((rc = check_audio("wun_sosfilt", n, C))) return rc;
    SosPlan p;
    if ((rc = sos_plan("wun_sosfilt", sos, nsec, &p))) return rc;
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x), ya = reinterpret_cast<uintptr_t>(y), bytes = (uintptr_t)n * C * 4;
    if (xa < ya + bytes && ya < xa + bytes) return fail(WUN_ERR_INVALID, "wun_sosfilt: x and y overlap (no in-place filtering)");

    hipStream_t s = (hipStream_t)stream;
    SosChunkArgs a;
    std::memset(&a, 0, sizeof(a));
    a.x = x; a.y = y;
    if (C == 2) launch_schedule<2, SOS_WRITE>(p, a, n, scratch, s);
    else launch_schedule<1, SOS_WRITE>(p, a, n, scratch, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(WUN_ERR_HIP, std::string("wun_sosfilt launch: ") + hipGetErrorString(e));
    return WUN_OK;
}

extern "C" int wun_kweight_design(int32_t sr, double* sos) {
    if (!sos) return fail(WUN_ERR_INVALID, "wun_kweight_design: null argument");
    if (sr < 4000 || sr > 384000) return fail(WUN_ERR_INVALID, "wun_kweight_design: sample rate outside 4000..384000 Hz");
    const double pi = 3.14159265358979323846;
    {   // stage 1: the high shelf
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / (double)sr), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        sos[0] = (Vh + Vb * K / Q + K * K) / a0;
        sos[1] = 2.0 * (K * K - Vh) / a0;
        sos[2] = (Vh - Vb * K / Q + K * K) / a0;
        sos[3] = 1.0;
        sos[4] = 2.0 * (K * K - 1.0) / a0;
        sos[5] = (1.0 - K / Q + K * K) / a0;
    }
    {   // stage 2: the high-pass, numerator not normalised
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / (double)sr);
        const double a0 = 1.0 + K / Q + K * K;
        sos[6] = 1.0; sos[7] = -2.0; sos[8] = 1.0;
        sos[9] = 1.0;
        sos[10] = 2.0 * (K * K - 1.0) / a0;
        sos[11] = (1.0 - K / Q + K * K) / a0;
    }
    return WUN_OK;
}

extern "C" int64_t wun_loudness_blocks(int64_t n, int32_t sr) {
    if (n < 1) return fail(WUN_ERR_INVALID, "wun_loudness_blocks: n < 1");
    if (sr < 4000 || sr > 384000) return fail(WUN_ERR_INVALID, "wun_loudness_blocks: sample rate outside 4000..384000 Hz");
    int64_t Nb, step, nb;
    block_geometry(sr, n, &Nb, &step, &nb);
    return nb;
}

extern "C" int64_t wun_loudness_scratch_doubles(int64_t n, int32_t C, int32_t sr) {
    int rc;
    if ((rc = check_audio("wun_loudness_scratch_doubles", n, C))) return rc;
    if (sr < 4000 || sr > 384000) return fail(WUN_ERR_INVALID, "wun_loudness_scratch_doubles: sample rate outside 4000..384000 Hz");
    int64_t Nb, step, nb;
    block_geometry(sr, n, &Nb, &step, &nb);
    return state_doubles(n, C, 2) + (int64_t)4 * C * n_chunks(n) + nb;       // states, pieces + peaks, z
}

extern "C" int wun_loudness(const float* x, int64_t n, int32_t C, int32_t sr, double* meter, double* blocks, double* scratch,
                            void* stream) {
    if (!x || !meter) return fail(WUN_ERR_INVALID, "wun_loudness: null argument");
    int rc;
    if ((rc = check_scratch("wun_loudness", scratch))) return rc;
    if (reinterpret_cast<uintptr_t>(meter) % 8 || reinterpret_cast<uintptr_t>(blocks) % 8)
        return fail(WUN_ERR_INVALID, "wun_loudness: meter / blocks are not 8-byte aligned");
    if ((rc = check_audio("wun_loudness", n, C))) return rc;
    double sos[12];
    if ((rc = wun_kweight_design(sr, sos))) return rc;
    SosPlan p;
    if ((rc = sos_plan("wun_loudness", sos, 2, &p))) return rc;
    int64_t Nb, step, nb;
    block_geometry(sr, n, &Nb, &step, &nb);

    hipStream_t s = (hipStream_t)stream;
    const long long nch = n_chunks(n);
    double* pieces = scratch + state_doubles(n, C, 2);
    double* peak = pieces + (long long)3 * C * nch;
    double* z = peak + (long long)C * nch;
    SosChunkArgs a;
    std::memset(&a, 0, sizeof(a));
    a.x = x; a.pieces = pieces; a.peak = peak; a.Nb = Nb; a.step = step;
    if (C == 2) launch_schedule<2, SOS_SQUARES>(p, a, n, scratch, s);
    else launch_schedule<1, SOS_SQUARES>(p, a, n, scratch, s);
    if (nb > 0)
        hipLaunchKernelGGL(loud_block_kernel, dim3((unsigned)((nb + WUN_LOUD_BLOCK - 1) / WUN_LOUD_BLOCK)), dim3(WUN_LOUD_BLOCK), 0, s,
                           pieces, z, (long long)n, nch, (long long)nb, (long long)Nb, (long long)step, (int)C);
    hipLaunchKernelGGL(loud_gate_kernel, dim3(1), dim3(WUN_LOUD_BLOCK), 0, s, z, (long long)nb, peak, (long long)C * nch, meter,
                       blocks);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(WUN_ERR_HIP, std::string("wun_loudness launch: ") + hipGetErrorString(e));
    return WUN_OK;
}

// ---- EBU R 128 ------------------------------------------------------------------------------------------
namespace {

int check_rate(const char* who, int32_t sr) {
    if (sr < 4000 || sr > 384000) return fail(WUN_ERR_INVALID, std::string(who) + ": sample rate outside 4000..384000 Hz");
    return WUN_OK;
}

int32_t peak_factor(int32_t sr) {
    int32_t L = 1;
    while (L < WUN_TP_MAXL && (int64_t)L * sr < 176400) L *= 2;
    return L;
}

bool peak_factor_ok(int32_t L) { return L >= 1 && L <= WUN_TP_MAXL && (L & (L - 1)) == 0; }

int64_t peak_groups(int64_t n) { return (n + WUN_TP_TILE - 1) / WUN_TP_TILE; }

void short_term_geometry(int32_t sr, int64_t n, int64_t* N3, int64_t* nb3) {
    *N3 = ((int64_t)30 * sr + 5) / 10;                     // round(3 sr), halves up, as Nb is formed
    const int64_t step = ((int64_t)sr + 5) / 10;
    *nb3 = n >= *N3 ? (n - *N3) / step + 1 : 0;
}

void launch_peak(const float* x, int64_t n, int32_t C, int32_t L, const float* table_dev, double* part, hipStream_t s) {
    PeakArgs a;
    a.x = x; a.taps = table_dev; a.part = part; a.n = n; a.L = L;
    const dim3 grid((unsigned)peak_groups(n)), blk(WUN_TP_BLOCK);
    if (C == 2) hipLaunchKernelGGL(true_peak_kernel<2>, grid, blk, 0, s, a);
    else hipLaunchKernelGGL(true_peak_kernel<1>, grid, blk, 0, s, a);
}

// the parts of wun_loudness_r128's scratch behind wun_loudness's own layout
struct R128Layout { int64_t pieces3, z3, key, small, part, total; };      // small: meter [4], mom [1], st [3], sel [2]

R128Layout r128_layout(int64_t n, int32_t C, int32_t sr) {
    int64_t Nb, step, nb, N3, nb3;
    block_geometry(sr, n, &Nb, &step, &nb);
    short_term_geometry(sr, n, &N3, &nb3);
    R128Layout l;
    l.pieces3 = state_doubles(n, C, 2) + (int64_t)4 * C * n_chunks(n) + nb;
    l.z3 = l.pieces3 + (int64_t)3 * C * n_chunks(n);
    l.key = l.z3 + nb3;
    l.small = l.key + nb3;
    l.part = l.small + 10;
    l.total = l.part + (int64_t)C * peak_groups(n);
    return l;
}

}  // namespace

extern "C" int32_t wun_true_peak_factor(int32_t sr) {
    int rc;
    if ((rc = check_rate("wun_true_peak_factor", sr))) return rc;
    return peak_factor(sr);
}

extern "C" int64_t wun_true_peak_scratch_doubles(int64_t n, int32_t C) {
    int rc;
    if ((rc = check_audio("wun_true_peak_scratch_doubles", n, C))) return rc;
    return (int64_t)C * peak_groups(n);
}

extern "C" int wun_true_peak(const float* x, int64_t n, int32_t C, int32_t L, const float* table_dev, double* out, double* scratch,
                             void* stream) {
    if (!x || !out) return fail(WUN_ERR_INVALID, "wun_true_peak: null argument");
    int rc;
    if ((rc = check_scratch("wun_true_peak", scratch))) return rc;
    if (reinterpret_cast<uintptr_t>(out) % 8) return fail(WUN_ERR_INVALID, "wun_true_peak: out is not 8-byte aligned");
    if ((rc = check_audio("wun_true_peak", n, C))) return rc;
    if (!peak_factor_ok(L)) return fail(WUN_ERR_INVALID, "wun_true_peak: L is not a power of two in 1..32 (wun_true_peak_factor)");
    if (L > 1 && !table_dev) return fail(WUN_ERR_INVALID, "wun_true_peak: null table (wun_resample_design(L, 1) on the device)");
    if (L > 1 && wun_resample_table_floats(L, 1) != (int64_t)L * WUN_TP_K)
        return fail(WUN_ERR_UNSUPPORTED, "wun_true_peak: the resampler's table no longer has 21 taps per phase");

    hipStream_t s = (hipStream_t)stream;
    launch_peak(x, n, C, L, table_dev, scratch, s);
    hipLaunchKernelGGL(true_peak_finish_kernel, dim3(1), dim3(WUN_LOUD_BLOCK), 0, s, scratch, (long long)peak_groups(n), (int)C, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(WUN_ERR_HIP, std::string("wun_true_peak launch: ") + hipGetErrorString(e));
    return WUN_OK;
}

extern "C" int64_t wun_loudness_short_term_blocks(int64_t n, int32_t sr) {
    if (n < 1) return fail(WUN_ERR_INVALID, "wun_loudness_short_term_blocks: n < 1");
    int rc;
    if ((rc = check_rate("wun_loudness_short_term_blocks", sr))) return rc;
    int64_t N3, nb3;
    short_term_geometry(sr, n, &N3, &nb3);
    return nb3;
}

extern "C" int64_t wun_loudness_r128_scratch_doubles(int64_t n, int32_t C, int32_t sr) {
    int rc;
    if ((rc = check_audio("wun_loudness_r128_scratch_doubles", n, C))) return rc;
    if ((rc = check_rate("wun_loudness_r128_scratch_doubles", sr))) return rc;
    return r128_layout(n, C, sr).total;
}

extern "C" int wun_loudness_r128(const float* x, int64_t n, int32_t C, int32_t sr, const float* table_dev, double* report,
                                 double* short_term, double* scratch, void* stream) {
    if (!x || !report) return fail(WUN_ERR_INVALID, "wun_loudness_r128: null argument");
    int rc;
    if ((rc = check_scratch("wun_loudness_r128", scratch))) return rc;
    if (reinterpret_cast<uintptr_t>(report) % 8 || reinterpret_cast<uintptr_t>(short_term) % 8)
        return fail(WUN_ERR_INVALID, "wun_loudness_r128: report / short_term are not 8-byte aligned");
    if ((rc = check_audio("wun_loudness_r128", n, C))) return rc;
    double sos[12];
    if ((rc = wun_kweight_design(sr, sos))) return rc;
    const int32_t L = peak_factor(sr);
    if (L > 1 && !table_dev) return fail(WUN_ERR_INVALID, "wun_loudness_r128: null table (wun_resample_design(L, 1) on the device)");
    if (L > 1 && wun_resample_table_floats(L, 1) != (int64_t)L * WUN_TP_K)
        return fail(WUN_ERR_UNSUPPORTED, "wun_loudness_r128: the resampler's table no longer has 21 taps per phase");
    SosPlan p;
    if ((rc = sos_plan("wun_loudness_r128", sos, 2, &p))) return rc;
    int64_t Nb, step, nb, N3, nb3;
    block_geometry(sr, n, &Nb, &step, &nb);
    short_term_geometry(sr, n, &N3, &nb3);
    if (nb3 > WUN_LRA_MAX_BLOCKS) return fail(WUN_ERR_UNSUPPORTED, "wun_loudness_r128: more than 2^20 short-term blocks");

    hipStream_t s = (hipStream_t)stream;
    const long long nch = n_chunks(n);
    const R128Layout l = r128_layout(n, C, sr);
    double* pieces = scratch + state_doubles(n, C, 2);                      // wun_loudness's layout, then the new parts
    double* peak = pieces + (long long)3 * C * nch;
    double* z = peak + (long long)C * nch;
    double* pieces3 = scratch + l.pieces3;
    double* z3 = scratch + l.z3;
    double* key = scratch + l.key;
    double* meter = scratch + l.small;
    double* mom = meter + 4;
    double* st = meter + 5;
    double* sel = meter + 8;
    double* part = scratch + l.part;
    SosChunkArgs a;
    std::memset(&a, 0, sizeof(a));
    a.x = x; a.pieces = pieces; a.peak = peak; a.pieces3 = pieces3; a.Nb = Nb; a.step = step; a.N3 = N3;
    if (C == 2) launch_schedule<2, SOS_SQUARES2>(p, a, n, scratch, s);
    else launch_schedule<1, SOS_SQUARES2>(p, a, n, scratch, s);
    const unsigned g = (unsigned)((nb + WUN_LOUD_BLOCK - 1) / WUN_LOUD_BLOCK), g3 = (unsigned)((nb3 + WUN_LOUD_BLOCK - 1) / WUN_LOUD_BLOCK);
    if (g + g3 > 0)
        hipLaunchKernelGGL(loud_block2_kernel, dim3(g + g3), dim3(WUN_LOUD_BLOCK), 0, s, pieces, z, (long long)nb, (long long)Nb,
                           pieces3, z3, (long long)nb3, (long long)N3, (long long)n, nch, (long long)step, (int)C, g);
    hipLaunchKernelGGL(r128_gate_kernel, dim3(2), dim3(WUN_LOUD_BLOCK), 0, s, z, (long long)nb, peak, (long long)C * nch, meter, mom,
                       z3, (long long)nb3, key, short_term, st);
    launch_peak(x, n, C, L, table_dev, part, s);
    if (g3 > 0) hipLaunchKernelGGL(lra_select_kernel, dim3(g3), dim3(WUN_LOUD_BLOCK), 0, s, key, (long long)nb3, st, sel);
    hipLaunchKernelGGL(r128_report_kernel, dim3(1), dim3(WUN_LOUD_BLOCK), 0, s, meter, mom, st, sel, part, (long long)peak_groups(n),
                       (int)C, report);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(WUN_ERR_HIP, std::string("wun_loudness_r128 launch: ") + hipGetErrorString(e));
    return WUN_OK;
}

extern "C" int wun_loudness_gain(const double* meter, double target_lufs, double max_gain_db, double peak_limit, float* gain,
                                 void* stream) {
    if (!meter || !gain) return fail(WUN_ERR_INVALID, "wun_loudness_gain: null argument");
    if (!std::isfinite(target_lufs)) return fail(WUN_ERR_INVALID, "wun_loudness_gain: target is not finite");
    if (!(max_gain_db >= 0.0) || !std::isfinite(max_gain_db)) return fail(WUN_ERR_INVALID, "wun_loudness_gain: max_gain_db < 0 or not finite");
    if (!(peak_limit >= 0.0) || !std::isfinite(peak_limit)) return fail(WUN_ERR_INVALID, "wun_loudness_gain: peak_limit < 0 or not finite (0: no limit)");
    hipLaunchKernelGGL(loud_gain_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, meter, target_lufs, max_gain_db, peak_limit, gain);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(WUN_ERR_HIP, std::string("wun_loudness_gain launch: ") + hipGetErrorString(e));
    return WUN_OK;
}

extern "C" int wun_scale_by(float* x, int64_t count, const float* gain, void* stream) {
    if (!x || !gain) return fail(WUN_ERR_INVALID, "wun_scale_by: null argument");
    if (count < 1) return fail(WUN_ERR_INVALID, "wun_scale_by: count < 1");
    int64_t blocks = (count + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(scale_by_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, (long long)count, gain);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(WUN_ERR_HIP, std::string("wun_scale_by launch: ") + hipGetErrorString(e));
    return WUN_OK;
}
