// train_kernels.hpp -- the statistics a probability table is trained from (picsong_train_*, gfx950): for every binary
// decision the two-pass coder (-cp 2, k = 0) would code in a Mallat coefficient array, one increment at
// counts[entry][symbol], entry = the table index the coder would read (raw index, clamped to the table as lut_at does).
// At k = 0 the (entry, symbol) sequence depends on the coefficients alone, so no table is read and nothing is coded.
//
// The coder's lock-step row scan exists for the arithmetic coder's slot order; the COUNTS need none of it.  What a
// coefficient sees is fixed by the data: a neighbour in the row above (and the left column of the same row, for a right
// column) is significant at the site iff it is significant AFTER this plane's significance pass, A | B; a neighbour
// below (and the other same-row ones) iff it was significant BEFORE it, A.  So a lane holds its two columns as 64-bit
// row masks exactly as the encoder does (enc_transpose_pass, the planes parked in the same scratch layout), forms the
// bit-sliced contexts of 32 rows at a time with the encoder's make_col, and counts with v_bcnt: per plane and column
// half 9 context selects, 4 sign-context selects and the refinement mask, two popcounts each.  No row loop, no serial
// chain, no interval arithmetic, no codeword reservation.
//
// Reduction on chip: a lane's 14 slots (9 significance contexts, 4 sign contexts, refinement; zeros | ones << 16, at most
// 128 a plane) go to a lane-private LDS column hist[slot * 64 + lane] -- conflict-free, no atomics; lanes 0..13 of a
// codeblock's half then sum one slot each over the half's 32 lanes (rotated, conflict-free) and add it into the
// workgroup's LDS copy of the whole counter array.  A codeblock whose lanes straddle subbands (per-lane groups) takes
// the slow path: every lane adds its own slots.  Workgroups are persistent over the codeblock pairs of all frames of a
// launch and leave with one 64-bit atomic add per non-zero counter.  Integer sums: the result is exact and
// independent of the order.
#pragma once
#include "bpc_kernels.hpp"

#ifndef __HIP_MEMORY_SCOPE_AGENT
#define __HIP_MEMORY_SCOPE_AGENT 4          // (CPU wave-emulator build: its atomics are plain read-modify-writes)
#endif

namespace picsong {

constexpr int kTrainWgWaves = 4;            // waves a workgroup; a wave takes a codeblock pair at a time
// entries of the counter array a workgroup can hold as uint32[entry][2] in LDS: 38 KB, + 3.5 KB a wave for the lane
// columns = 52 KB, three workgroups a CU.  wl <= 7 at 15 / 3 / 1 / 4 / 9: 15 * 22 * 14 = 4620.
constexpr int kTrainMaxEntries = 4864;
constexpr int kTrainSlots = 14;             // 9 significance contexts, 4 sign contexts, refinement
constexpr unsigned kTrainMaxWgs = 768;      // persistent grid: three workgroups a CU of 256
// A workgroup's uint32 copy cannot overflow: an entry takes at most 2 * 4096 increments a codeblock (two bit-planes may
// alias onto one entry), a launch covers at most 64 frames of 2^30 / 4096 codeblocks, the grid has `wgs` workgroups
// of 4 waves -- a wave sees <= ceil(2^23 / (4 wgs)) pairs; the host keeps that below 2^32 / 2^14 (train_pairs_ok).
inline bool train_pairs_ok(size_t pairs, unsigned wgs)
{
    const size_t per_wave = (pairs + (size_t)wgs * kTrainWgWaves - 1) / ((size_t)wgs * kTrainWgWaves);
    return per_wave * (size_t)kTrainWgWaves <= ((size_t)1 << 18);
}

// the counts of one column half (32 rows): ins = not yet significant, sig = significant before this plane,
// b = the plane's bits; tot / one: per slot, symbols and ones among them
__device__ __forceinline__ void train_count_col(const ColHalf &cp, uint32_t ins, uint32_t sig, uint32_t b,
                                                uint32_t (&tot)[kTrainSlots], uint32_t (&one)[kTrainSlots])
{
    const uint32_t lo = ins & ~cp.n3;
    const uint32_t a0 = lo & ~cp.n0, a1 = lo & cp.n0;
    const uint32_t q[4] = { a0 & ~cp.n1, a1 & ~cp.n1, a0 & cp.n1, a1 & cp.n1 };      // context bits 1..0
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t sel = (k & 4) ? (q[k & 3] & cp.n2) : (q[k & 3] & ~cp.n2);
        tot[k] = bcnt_acc(sel, tot[k]);
        one[k] = bcnt_acc(sel & b, one[k]);
    }
    const uint32_t s8 = ins & cp.n3;
    tot[8] = bcnt_acc(s8, tot[8]);
    one[8] = bcnt_acc(s8 & b, one[8]);
    // the sign of a coefficient that becomes significant: table index c >> 1 = c2 c1, symbol = sign ^ c0
    const uint32_t nw = ins & b;
    const uint32_t g0 = nw & ~cp.c1, g1 = nw & cp.c1;
    const uint32_t sg[4] = { g0 & ~cp.c2, g1 & ~cp.c2, g0 & cp.c2, g1 & cp.c2 };
#pragma unroll
    for (int j = 0; j < 4; j++) {
        tot[9 + j] = bcnt_acc(sg[j], tot[9 + j]);
        one[9 + j] = bcnt_acc(sg[j] & cp.s2, one[9 + j]);
    }
    tot[13] = bcnt_acc(sig, tot[13]);
    one[13] = bcnt_acc(sig & b, one[13]);
}

// the table entry of slot s for group base G (level * nSub * nBp + sb * nBp) and bit-plane bp, as lut_at clamps it
__device__ __forceinline__ int train_entry(const LutGeo &g, int total, int G, int bp, int s)
{
    int e;
    if (s < 9) e = g.nRef + (G + bp) * g.cSig + s;
    else if (s < 13) e = g.nRef + g.nSig + (G + bp) * g.cSign + (s - 9);
    else e = (G + bp) * g.cRef;
    return e < 0 ? 0 : (e >= total ? total - 1 : e);
}

// a: the encoder's arguments for the coefficient side (coeffs_in, is_float, c16, AW, AH, wl, ncx, nCB, g, range_flag,
// coef_z; waves_per_frame = the codeblock pairs of a frame; plane_scratch: kEncScratchDwordsPerWave per wave of the
// grid).  pairs: codeblock pairs of the launch, all frames.  counts: uint64[nRef + nSig + nSign][2], added to.
__global__ __launch_bounds__(64 * kTrainWgWaves) void bpc_stats_kernel(BpcArgs a, unsigned long long *counts, int pairs)
{
    __shared__ uint32_t wg_cnt[kTrainMaxEntries * 2];
    __shared__ uint32_t lane_hist[kTrainWgWaves * kTrainSlots * 64];
    const int total = a.g.nRef + a.g.nSig + a.g.nSign;
    if (total > kTrainMaxEntries) return;                    // (the host refuses such a geometry: picsong_train_begin)
    for (int i = (int)threadIdx.x; i < 2 * total; i += (int)blockDim.x) wg_cnt[i] = 0u;
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u, half = lane >> 5, t = lane & 31u;
    const int wv = (int)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gwave = (int)blockIdx.x * kTrainWgWaves + wv, nwaves = (int)gridDim.x * kTrainWgWaves;
    const uint32_t upper_mask = opaque_mask(half ? 0xFFFFFFFFu : 0u);
    uint32_t *const pscr = a.plane_scratch + (size_t)gwave * (size_t)kEncScratchDwordsPerWave + lane;
    uint32_t *const hist = lane_hist + wv * (kTrainSlots * 64);
    const char *const coef0 = reinterpret_cast<const char *>(a.coeffs_in);
    const uint32_t esz = a.c16 ? 2u : 4u, rstride = (uint32_t)a.AW * esz;

#pragma unroll 1
    for (int pair = gwave; pair < pairs; pair += nwaves) {   // wave-uniform
        const int f = pair / a.waves_per_frame, wave = pair - f * a.waves_per_frame;
        a.coeffs_in = coef0 + (unsigned long long)f * a.coef_z;
        const int cb = 2 * wave + (int)half;
        const bool valid = cb < a.nCB;
        const int cbx = valid ? cb % a.ncx : 0, cby = valid ? cb / a.ncx : 0;
        const size_t cbase = (size_t)(cby * 64) * (size_t)a.AW + (size_t)(cbx * 64) + 2u * t;
        const uint32_t cbyte = (uint32_t)cbase * esz;

        // ---- the encoder's pass over the coefficients: MSB, sign masks, the planes' row masks into the scratch
        U64 sgL = { 0u, 0u }, sgR = { 0u, 0u };
        uint32_t ormag = 0u;
        int msb = 32, msbmax = -1;
        bool coded = false;
#pragma unroll 1
        for (int pass = 0; pass < kMaxPlanes / kEncPassPlanes; pass++) {
            if (valid) {
                if (a.c16) enc_transpose_pass<2>(a, pass, cbyte, rstride, pscr, ormag, sgL, sgR);
                else if (a.is_float) enc_transpose_pass<1>(a, pass, cbyte, rstride, pscr, ormag, sgL, sgR);
                else enc_transpose_pass<0>(a, pass, cbyte, rstride, pscr, ormag, sgL, sgR);
            }
            if (pass == 0) {
                ormag = half_or_dpp(ormag, upper_mask);
                msb = ormag ? 31 - __builtin_clz(ormag) : 32;
                // a codeblock beyond the table's bit-planes contributes nothing
                if (valid && msb != 32 && msb > kMaxPlanes - 1) { atomicOr(a.range_flag, 1); msb = 32; }
                coded = valid && msb != 32;
                int mm = coded ? msb : -1;
                { int o = __shfl_xor(mm, 32); mm = mm > o ? mm : o; }
                msbmax = (int)__builtin_amdgcn_readfirstlane((uint32_t)mm);
            }
            if (msbmax < (pass + 1) * kEncPassPlanes) break;
        }

        int level, sb;
        find_subband_sel(cbx * 64 + 2 * (int)t, cby * 64, a.AW, a.AH, a.wl, level, sb);
        const int G = (level * a.g.nSub + sb) * a.g.nBp;
        // does a half's group differ between its lanes?  (codeblocks that straddle subbands at the coarse levels)
        const int Gp = (int)dpp_prev((uint32_t)G);
        const uint64_t dm = __builtin_amdgcn_ballot_w64(t != 0u && Gp != G);
        const bool mixed = (half ? (uint32_t)(dm >> 32) : (uint32_t)dm) != 0u;
        const int np = msbmax + 1;                           // wave-uniform

        U64 AL = { 0u, 0u }, AR = { 0u, 0u };                // significant before the current plane
#pragma unroll 1
        for (int p = 0; p < np; p++) {
            const int bp = msb - p;                          // the lane's codeblock's own plane
            const bool act = coded && bp >= 0;
            U64 BL = { 0u, 0u }, BR = { 0u, 0u };
            if (act) {
                const uint32_t *q = pscr + (size_t)bp * kEncPlaneDwords;
                BL.lo = q[0]; BL.hi = q[64]; BR.lo = q[128]; BR.hi = q[192];
            }
            const U64 AL2 = u_or(AL, BL), AR2 = u_or(AR, BR);          // state after this plane's significance pass
            const U64 sgPL = u_prev(sgR, t), sgNL = u_next(sgL, t);    // neighbour sign columns
            const U64 APL = u_prev(AR, t), APL2 = u_prev(AR2, t);      // lane-1's right column
            const U64 ANL = u_next(AL, t), ANL2 = u_next(AL2, t);      // lane+1's left column
            uint32_t tot[kTrainSlots], one[kTrainSlots];
#pragma unroll
            for (int s = 0; s < kTrainSlots; s++) { tot[s] = 0u; one[s] = 0u; }
#pragma unroll
            for (int hw = 0; hw < 2; hw++) {
                const ColHalf cpL = make_col(up_of(APL2, hw), up_of(AL2, hw), up_of(AR2, hw), w_of(APL, hw), w_of(AR, hw),
                                             dn_of(APL, hw), dn_of(AL, hw), dn_of(AR, hw),
                                             up_of(AL2, hw), up_of(sgL, hw), dn_of(AL, hw), dn_of(sgL, hw),
                                             w_of(APL, hw), w_of(sgPL, hw), w_of(AR, hw), w_of(sgR, hw), w_of(sgL, hw));
                const ColHalf cpR = make_col(up_of(AL2, hw), up_of(AR2, hw), up_of(ANL2, hw), w_of(AL2, hw), w_of(ANL2, hw),
                                             dn_of(AL, hw), dn_of(AR, hw), dn_of(ANL, hw),
                                             up_of(AR2, hw), up_of(sgR, hw), dn_of(AR, hw), dn_of(sgR, hw),
                                             w_of(AL2, hw), w_of(sgL, hw), w_of(ANL2, hw), w_of(sgNL, hw), w_of(sgR, hw));
                const uint32_t al = w_of(AL, hw), ar = w_of(AR, hw);
                train_count_col(cpL, act ? ~al : 0u, act ? al : 0u, w_of(BL, hw), tot, one);
                train_count_col(cpR, act ? ~ar : 0u, act ? ar : 0u, w_of(BR, hw), tot, one);
            }
            AL = AL2; AR = AR2;

            // ---- the plane's 14 slots of every lane -> the workgroup's copy
#pragma unroll
            for (int s = 0; s < kTrainSlots; s++) hist[s * 64 + (int)lane] = (tot[s] - one[s]) | (one[s] << 16);
            wave_lds_done();
            if (act && !mixed && t < (uint32_t)kTrainSlots) {
                const uint32_t *row = hist + t * 64u + half * 32u;
                uint32_t sum = 0u;
#pragma unroll 8
                for (uint32_t j = 0; j < 32u; j++) sum += row[(j + t) & 31u];
                const int e = train_entry(a.g, total, G, bp, (int)t);
                if (sum & 0xFFFFu) atomicAdd(&wg_cnt[2 * e], sum & 0xFFFFu);
                if (sum >> 16) atomicAdd(&wg_cnt[2 * e + 1], sum >> 16);
            }
            if (act && mixed) {
#pragma unroll
                for (int s = 0; s < kTrainSlots; s++) {
                    const int e = train_entry(a.g, total, G, bp, s);
                    if (tot[s] != one[s]) atomicAdd(&wg_cnt[2 * e], tot[s] - one[s]);
                    if (one[s]) atomicAdd(&wg_cnt[2 * e + 1], one[s]);
                }
            }
            wave_lds_done();                                 // the columns are free for the next plane
        }
    }

    __syncthreads();
    for (int i = (int)threadIdx.x; i < 2 * total; i += (int)blockDim.x) {
        const uint32_t v = wg_cnt[i];
        if (v) (void)__hip_atomic_fetch_add(&counts[i], (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace picsong
