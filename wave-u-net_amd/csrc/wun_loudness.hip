// gfx950 (MI355X / CDNA4): recursive (IIR) filtering along time and the BS.1770-4 loudness meter built on it
// (include/wun.h: wun_sosfilt, wun_kweight_design, wun_loudness, wun_loudness_gain, wun_scale_by).
//
//   biquad cascade     y = sosfilt(sos, x) per channel from zero initial state, direct form I per section:
//                      y[t] = b0 x[t] + b1 x[t-1] + b2 x[t-2] - a1 y[t-1] - a2 y[t-2]      (float64, rounded once to float32)
//   loudness           K-weighting (two sections), mean squares over blocks of 0.4 s at a step of 0.1 s, absolute gate at
//                      -70 LUFS, relative gate 10 LU under the absolute-gated mean; the filtered signal is never written
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

enum { SOS_END_STATE = 0, SOS_WRITE = 1, SOS_SQUARES = 2 };

struct SosChunkArgs {
    const float* x; float* y;        // [n, C]; y: SOS_WRITE only
    double* st;                      // [2 nsec][C][nchunks] end states e_k: SOS_END_STATE writes them, the other modes read them
    double* grp;                     // [2 nsec][C][ngroups]: SOS_END_STATE writes the group ends, the other modes read the group starts
    double* pieces;                  // SOS_SQUARES: [3][C][nchunks] sums of squares of the chunk's pieces
    double* peak;                    // SOS_SQUARES: [C][nchunks] max |x| of the chunk (NaN if it holds one)
    long long n, nchunks, ngroups, Nb, step;
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
    long long c1 = 0, c2 = 0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, pk = 0.0;
    if (MODE == SOS_SQUARES) {
        const long long t1 = t0 + WUN_SOS_CHUNK < p.n ? t0 + WUN_SOS_CHUNK : p.n;
        loud_cuts(t0, t1, p.Nb, p.step, c1, c2);
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
                if (MODE == SOS_SQUARES) {
                    if (t < c1) a0 = fma(yv, yv, a0);
                    else if (t < c2) a1 = fma(yv, yv, a1);
                    else a2 = fma(yv, yv, a2);
                    pk = nan_max(pk, fabs((double)xf));
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
    if (MODE == SOS_SQUARES && live) {
        p.pieces[((long long)0 * CH + c) * p.nchunks + kc] = a0;
        p.pieces[((long long)1 * CH + c) * p.nchunks + kc] = a1;
        p.pieces[((long long)2 * CH + c) * p.nchunks + kc] = a2;
        p.peak[(long long)c * p.nchunks + kc] = pk;
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
__global__ __launch_bounds__(WUN_LOUD_BLOCK) void loud_block_kernel(const double* __restrict__ pieces, double* __restrict__ z,
                                                                    long long n, long long nchunks, long long nb, long long Nb,
                                                                    long long step, int C) {
    const long long j = (long long)blockIdx.x * WUN_LOUD_BLOCK + threadIdx.x;
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
__global__ __launch_bounds__(WUN_LOUD_BLOCK) void loud_gate_kernel(const double* __restrict__ z, long long nb,
                                                                   const double* __restrict__ peak, long long npeak,
                                                                   double* __restrict__ meter, double* __restrict__ blocks) {
    __shared__ double red[WUN_LOUD_BLOCK];
    const int tid = threadIdx.x;
    double sum = 0.0, cnt = 0.0, bad = 0.0;
    for (long long j = tid; j < nb; j += WUN_LOUD_BLOCK) {
        const double l = loud_lufs(z[j]);
        if (blocks) blocks[j] = l;
        if (l != l) bad = 1.0;
        if (l > -70.0) { sum += z[j]; cnt += 1.0; }
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
