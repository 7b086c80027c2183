// launch_plan.hpp -- host-side launch geometry for the per-level DWT kernels (pure host code,
// shared by the C-ABI implementation and by the CPU wave-emulator tests so both walk the levels
// the same way; launch_seq.hpp launches the plans).  Level order and scratch offsets follow DWTEngine::DWTForward / DWTReverse
// (reference DWT/DWTGenerator.cu:1268-1424).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <cmath>
#include <vector>

#include "dwt_kernels.hpp"

namespace picsong {

// DWT/DWTGenerator.cuh:168-179 -- quantisation steps, columns LL,HL,LH,HH, row = level
static const float kQSteps[10][4] = {
    { 1.965908f, 1.0112865f, 1.0112865f, 0.52021784f },
    { 4.1224113f, 1.9968134f, 1.9968134f, 0.96721643f },
    { 8.416739f, 4.1833673f, 4.1833673f, 2.0792568f },
    { 16.935543f, 8.534108f, 8.534108f, 4.3004827f },
    { 33.924816f, 17.166693f, 17.166693f, 8.686718f },
    { 67.87687f, 34.385098f, 34.385098f, 17.41882f },
    { 135.76744f, 68.7964f, 68.7964f, 34.860676f },
    { 271.5416f, 137.60588f, 137.60588f, 69.73287f },
    { 543.0866f, 275.21814f, 275.21814f, 139.47136f },
    { 1086.1624f, 550.43286f, 550.43286f, 278.94202f }
};

// u16 (deep contexts, level 0 only): the input is uint16 samples (select_fwd: the U16IN instantiations); false: as ever
// rgb16 (deep RGB contexts, level 0 only): the input is three uint16 planes a frame, the colour transform in the load stage,
// grid.z = 3 n planes (select_fwd: the RGB16 instantiations); false: as ever
struct FwdLaunch { DwtFwdArgs a; unsigned gx, gy; bool u8; int band; bool vec; bool u16; bool rgb16; };
struct InvLaunch { DwtInvArgs a; unsigned gx, gy; int band; bool vec; bool fast; };

// The vector-only kernel instantiations need whole 4-column groups and 16-byte aligned rows
// (PICSONG_DWT_NOVEC=1 forces the per-column kernels, used by the tests to cross-check both).
inline bool dwt_vec_ok(int W, int aw, const void *p0, const void *p1)
{
    if (const char *e = getenv("PICSONG_DWT_NOVEC")) if (atoi(e) != 0) return false;
    return W >= 4 && (W & 3) == 0 && (aw & 3) == 0 && (((uintptr_t)p0 | (uintptr_t)p1) & 15u) == 0;
}

// Band height per level: big levels want taller bands (less vertical halo re-read), small levels
// want many short waves (a level with a handful of tall waves is bound by one wave's serial
// instruction time, not by memory); PICSONG_DWT_BANDS="16,8,4,..." overrides per level.
// tests/test_dwt_bands.py and tests/test_dwt_bands_gpu.py rely on the override (read at every plan) to run the 8-, 16-
// and 32-row instantiations at small frames.
inline int band_rows_override(int level)
{
    if (const char *e = getenv("PICSONG_DWT_BANDS")) {
        int l = 0;
        for (const char *p = e; *p; l++) {
            int v = atoi(p);
            if (l == level && (v == 4 || v == 8 || v == 16 || v == 32)) return v;
            while (*p && *p != ',') p++;
            if (*p == ',') p++;
        }
    }
    return 0;
}
inline int fwd_band_rows(int level, int strips, int H)
{
    if (const int v = band_rows_override(level)) return v;
    // measured on MI355X (8K: 16,8,4,4,4 best; 4K: 8,8,4,4,4): by level size in samples
    const long n = (long)H * (long)strips * kStripUseful;
    return n >= (16L << 20) ? 16 : (n >= (4L << 20) ? 8 : 4);
}
// The 9/7 synthesis of a context whose reciprocal divisions verified (dwt_inv97_kernel) is bound by its vector
// instructions, a third of which a 16-row band spends on run-in rows (12 iterations for 8 row pairs; 32 rows: 20
// for 16): taller bands than the other kernels want.  Measured on an 8K frame, wl = 6 (round 2):
// 32,16,8,4,4,4 rows for levels 0..5 81.1 us; 32,8,4,4,4,4 83.9; 16,8,4,4,4,4 95.2; 32-row bands on level 1
// double level 0's time (38.7 -> 76.5 us; same words out).
inline int inv97_band_rows(int level, int strips, int H)
{
    if (const int v = band_rows_override(level)) return v;
    const long n = (long)H * (long)strips * kStripUseful;
    return n >= (16L << 20) ? 32 : (n >= (4L << 20) ? 16 : (n >= (1L << 20) ? 8 : 4));
}

// -k > 0: bytes the COMPACT table copy of the frame's widest codeblock needs (bulk_setup<true>, bpc_kernels.hpp): the
// groups g0 .. g1 its 32 lanes' subbands span (findSubband BPC/BPCEngine.cu:143-170 at x = 64 cbx + 2 t, y = 64 cby), of
// the three sections, each with its slack planes.  A function of the geometry alone; the host takes the COMPACT
// instantiations of the -k > 0 kernels when it is at most kBulkCompactBytes.
inline int bulk_max_span_bytes(int aw, int ah, int wl, int nBp, int nSub, int cRef, int cSig, int cSign)
{
    auto group = [&](int x, int y) {
        for (int a = 1; a <= wl; a++) {
            const bool cx = x >= (aw >> a), cy = y >= (ah >> a);
            if (cx || cy) return (a - 1) * nSub + (cx ? (cy ? 2 : 0) : 1);
        }
        return wl * nSub;
    };
    int worst = 1;
    for (int cby = 0; cby < ah / 64; cby++)
        for (int cbx = 0; cbx < aw / 64; cbx++) {
            int g0 = 1 << 30, g1 = -1;
            for (int t = 0; t < 32; t++) { const int g = group(cbx * 64 + 2 * t, cby * 64); g0 = g < g0 ? g : g0; g1 = g > g1 ? g : g1; }
            worst = g1 - g0 + 1 > worst ? g1 - g0 + 1 : worst;
        }
    const int sl = nBp < 15 ? 16 - nBp : 1;
    return (worst * nBp + sl) * (cRef + cSig + cSign);
}

// May the frame paths carry their coded coefficients as 16-bit integers (DwtFwdArgs::c16)?  The largest magnitude a
// subband sample can take is  max|sample| x G_x x G_y  x (9/7: the quantisation weight QSTEP[l][sb] x qs), G = the L1
// gain of the multi-level 1-D analysis from the input to a level's low / high output: at most 1.3803 / 2.6253 for the
// 9/7 transform as implemented here, 1.7141 / 2.8601 for 5/3 whatever the level (tools/dwt_gain_bounds.py applies the
// transforms to the identity; the 5/3 floors move a sample by less than one per lifting step).  `in_max`: largest
// sample magnitude after the level shift / colour transform (128 for a grey 8-bit frame, 255 for RCT chroma).
// 2^15 with a margin for rounding; PICSONG_C16=0 keeps the 32-bit arrays (the tests cross-check both).
// coef16_bound: the bound alone, whatever the environment says (picsong_depth_range_guaranteed)
inline bool coef16_bound(bool lossy, int wl, float qs, int in_max)
{
    if (wl < 1 || wl > 10) return false;
    if (!lossy) return (double)in_max * 2.8601 * 2.8601 + 64.0 < 30000.0;
    if (!(qs > 0.0f)) return false;
    const double gl = 1.3803, gh = 2.6253, g[4] = { gl * gl, gl * gh, gl * gh, gh * gh };
    double worst = 0.0;
    for (int l = 0; l < wl; l++)
        for (int k = (l == wl - 1 ? 0 : 1); k < 4; k++) {
            const double b = (double)in_max * g[k] * (double)kQSteps[l][k] * (double)qs;
            worst = b > worst ? b : worst;
        }
    return worst < 30000.0;
}
inline bool coef16_ok(bool lossy, int wl, float qs, int in_max)
{
    if (const char *e = getenv("PICSONG_C16")) if (atoi(e) == 0) return false;
    return coef16_bound(lossy, wl, qs, in_max);
}

inline std::vector<FwdLaunch> plan_dwt_forward(const void *d_in, bool u8in, void *d_out, int aw, int ah,
                                               int wl, float qs, bool c16 = false)
{
    std::vector<FwdLaunch> v;
    int W = aw, H = ah;
    size_t off = 0;
    const char *src = (const char *)d_in;
    int src_stride = aw;
    for (int l = 0; l < wl; l++) {
        const bool last = (l == wl - 1);
        off += (size_t)W * (size_t)H;
        FwdLaunch f;
        DwtFwdArgs &a = f.a;
        a.src = src; a.src_stride = src_stride; a.W = W; a.H = H;
        a.ll = last ? d_out : (void *)((char *)d_out + off * 4);
        a.ll_stride = last ? aw : (W >> 1);
        a.mallat = d_out; a.AW = aw; a.level = l; a.last = last ? 1 : 0; a.qs = qs;
        a.src_z = 0; a.dst_z = 0; a.pair_base = 0; a.pair_end = 0; a.c16 = c16 ? 1 : 0;
        a.src_g = a.src_b = nullptr; a.off = 0;
        for (int k = 0; k < 4; k++) a.q[k] = kQSteps[l][k];
        const int strips = (W + kStripUseful - 1) / kStripUseful;
        f.band = fwd_band_rows(l, strips, H);
        f.gx = (unsigned)((strips + 3) / 4);
        f.gy = (unsigned)(((H >> 1) + f.band / 2 - 1) / (f.band / 2));
        f.u8 = u8in && l == 0;
        f.u16 = false;
        f.rgb16 = false;
        // rows of every buffer this level touches start 16-byte aligned when W % 4 == 0: strides are
        // aw, W or W/2 (even), scratch offsets are sums of W*H (multiples of 16 elements)
        f.vec = dwt_vec_ok(W, aw, d_in, d_out) && (W >> 1) % 2 == 0;
        v.push_back(f);
        src = (const char *)d_out + off * 4;
        src_stride = W >> 1;
        W >>= 1; H >>= 1;
    }
    // (the 16-bit form exists in the vector-only kernel instantiations: every level or none)
    bool all_vec = true;
    for (const FwdLaunch &f : v) all_vec = all_vec && f.vec;
    if (!all_vec) for (FwdLaunch &f : v) f.a.c16 = 0;
    return v;
}
inline bool plan_is_c16(const std::vector<FwdLaunch> &plan) { return !plan.empty() && plan[0].a.c16 != 0; }

// ---- deep contexts (bit_depth 9..16, grey, the 32-bit coefficient form): the two ends of the transform on uint16 samples.
// PICSONG_DEEP_NOFUSE=1 (read per call): the element-wise level shift / clamp passes beside the T-input level 0 and the
// T-output finest level, instead of the uint16 load and store stages of the kernels.  The bytes are the same.
inline bool deep_nofuse()
{
    const char *e = getenv("PICSONG_DEEP_NOFUSE");
    return e && atoi(e) != 0;
}
inline bool deep_depth_ok(int bit_depth) { return bit_depth >= 9 && bit_depth <= 16; }
// The forward plan of n frames of uint16 samples at d_in, frame_stride bytes apart: level 0 reads the samples itself
// (FwdLaunch::u16), level shift `off` = 2^(bit depth - 1) -- its vector form where the plan's level 0 has it and the frames
// start 16-byte aligned (stride included), its per-column form otherwise.  Never the 16-bit coefficient form, never the
// fused head (plan_dwt_fwd2 wants a u8 level 0).
inline std::vector<FwdLaunch> plan_dwt_forward_u16(const uint16_t *d_in, size_t frame_stride, unsigned frames, void *d_out, int aw, int ah,
                                                   int wl, float qs, int off)
{
    std::vector<FwdLaunch> v = plan_dwt_forward(d_in, false, d_out, aw, ah, wl, qs, false);
    v[0].u16 = true;
    v[0].a.off = off;
    if (frames > 1 && (frame_stride & 15u)) v[0].vec = false;
    return v;
}

// ... of n deep RGB frames: three uint16 planes a frame at d_r / d_g / d_b, frame f's frame_stride bytes behind.  Level 0
// reads them and applies the colour transform itself (FwdLaunch::rgb16, grid.z = 3 n): its vector form where the plan's
// level 0 has it, all three planes start 16-byte aligned and frame_stride is a multiple of 16; its per-column form
// otherwise.  A lane holds six dwords a raw row, three times the grey stage's: the vector form keeps every band height's
// rows in registers; the per-column form, whose mirrored addresses cost registers too, does so up to 8 rows (at 16 and 32
// its instantiations spill into accumulation registers at one wave a SIMD: DESIGN.md 4.19), so it takes at most 8.
constexpr int kRgb16ColumnMaxBand = 8;
inline std::vector<FwdLaunch> plan_dwt_forward_rgb16(const uint16_t *d_r, const uint16_t *d_g, const uint16_t *d_b, size_t frame_stride,
                                                     unsigned frames, void *d_out, int aw, int ah, int wl, float qs, int off)
{
    std::vector<FwdLaunch> v = plan_dwt_forward_u16(d_r, frame_stride, frames, d_out, aw, ah, wl, qs, off);
    FwdLaunch &f = v[0];
    f.u16 = false; f.rgb16 = true;
    f.a.src_g = d_g; f.a.src_b = d_b;
    if ((((uintptr_t)d_r) | ((uintptr_t)d_g) | ((uintptr_t)d_b)) & 15u) f.vec = false;
    if (!f.vec && f.band > kRgb16ColumnMaxBand) {
        f.band = kRgb16ColumnMaxBand;
        f.gy = (unsigned)(((ah >> 1) + f.band / 2 - 1) / (f.band / 2));
    }
    return v;
}

// The UNQUANTISED 9/7 transform of the rate calls (picsong_encode_frame_rate): the same plan with every step and qs at
// 1.0f -- x * 1.0f * 1.0f is x, the transform is exact -- in the 32-bit float form, so one frame lands in one float
// Mallat array at d_out (the last level's LL in its corner as usual).  quantise_kernel (rate_kernels.hpp) makes the
// coefficients of any qs from it.
inline std::vector<FwdLaunch> plan_dwt_forward_unit(const void *d_in, bool u8in, void *d_out, int aw, int ah, int wl)
{
    std::vector<FwdLaunch> v = plan_dwt_forward(d_in, u8in, d_out, aw, ah, wl, 1.0f, false);
    for (FwdLaunch &f : v)
        for (int k = 0; k < 4; k++) f.a.q[k] = 1.0f;
    return v;
}

// Level 0 restricted to the input rows [row0, row0 + rows) (both even): the launch then produces the row
// pairs [row0 / 2, (row0 + rows) / 2) of HL / LH / HH (Mallat) and of LL (scratch, or Mallat when wl = 1).
inline void plan_restrict_band(FwdLaunch &f, int row0, int rows)
{
    f.a.pair_base = row0 >> 1;
    f.a.pair_end = (row0 + rows) >> 1;
    f.gy = (unsigned)(((rows >> 1) + f.band / 2 - 1) / (f.band / 2));
}

// May the 9/7 synthesis of a context with this qs use the reciprocal form of its divisions
// (div_rc, dwt_kernels.hpp)?  Checks, with the very arithmetic the kernels run, every value the
// de-quantisation can see: m = |v| + 0.5 for |v| < 65536 (16 bit-planes) over each quantisation step
// q of the wl levels, m / q == div_rc(m, q) and (m / q) / qs == div_rc(m / q, qs).  ~3 M divisions,
// a few milliseconds, once per context.  PICSONG_DWT_EXACTDIV=1 forces the dividing kernels.
inline bool dequant_fast_ok(float qs, int wl)
{
    if (const char *e = getenv("PICSONG_DWT_EXACTDIV")) if (atoi(e) != 0) return false;
    if (!(qs >= 0x1p-20f && qs <= 0x1p20f)) return false;
    const volatile float one = 1.0f;                      // the reciprocals stay IEEE divisions at -O3 too
    const float rqs = one / qs;
    float seen[40];
    int nseen = 0;
    for (int l = 0; l < wl && l < 10; l++)
        for (int k = 0; k < 4; k++) {
            const float q = kQSteps[l][k];
            bool dup = false;
            for (int i = 0; i < nseen; i++) dup = dup || seen[i] == q;
            if (dup) continue;
            seen[nseen++] = q;
            const float rq = one / q;
            for (int n = 0; n < 65536; n++) {
                const float m = (float)n + 0.5f;
                const float t = m / q;
                if (div_rc(m, q, rq) != t || div_rc(t, qs, rqs) != t / qs) return false;
            }
        }
    return true;
}

// Levels 0 and 1 of a forward plan as ONE launch of dwt_fwd2_kernel (dwt_kernels.hpp): the frame path
// (u8 input: a band's 41-53 rows fit the registers as one dword each), both levels on the vector path,
// enough rows for the mirrored run-in.  `wanted`: the context's choice (not when it is told that other
// frames share the GPU, picsong_ctx_set_pipelined); PICSONG_DWT_NOFUSE01=1 / PICSONG_DWT_FUSE01=1 force
// two launches / the fused one (the tests cross-check both).
struct Fwd2Launch { DwtFwd2Args a; unsigned gx, gy; };
// nb_override > 0: level-1 row pairs per band (the RGB head: kF2PairsRgb)
inline bool plan_dwt_fwd2(const std::vector<FwdLaunch> &plan, Fwd2Launch &f, bool wanted = true, bool lossy = false,
                          int nb_override = 0)
{
    if (const char *e = getenv("PICSONG_DWT_NOFUSE01")) if (atoi(e) != 0) return false;
    if (const char *e = getenv("PICSONG_DWT_FUSE01")) wanted = wanted || atoi(e) != 0;
    if (!wanted) return false;
    if (plan.size() < 2 || !plan[0].vec || !plan[1].vec || !plan[0].u8) return false;
    const DwtFwdArgs &l0 = plan[0].a;
    if (l0.H < 64 || (l0.H & 3) || l0.W < 8 || (l0.W & 7)) return false;
    const int pairs1 = l0.H >> 2;                                   // level-1 row pairs
    f.a.l0 = l0; f.a.l1 = plan[1].a;
    const int strips = (l0.W + kF2Useful - 1) / kF2Useful;
    f.gx = (unsigned)((strips + 3) / 4);
    const int nb = nb_override > 0 ? nb_override : (lossy ? kF2PairsLossy : kF2Pairs);
    if (pairs1 % nb) return false;                                  // whole bands only (dwt_fwd2_band)
    f.gy = (unsigned)((pairs1 + nb - 1) / nb);
    return true;
}

// nb_override of a call that carries `frames` frames: the 5/3 int16 head's longer bands (kF2PairsBatch) where a call has
// more than one frame and the level-1 row pairs are whole bands of that length; 0 = the transform's own band length
inline int f2_pairs_batched(const std::vector<FwdLaunch> &plan, bool lossy, unsigned frames)
{
    if (lossy || frames < 2 || kF2PairsBatch == kF2Pairs || !plan_is_c16(plan)) return 0;
    return ((plan[0].a.H >> 2) % kF2PairsBatch) == 0 ? kF2PairsBatch : 0;
}

// the 16-bit form exists in the vector-only kernel instantiations: every level of the frame on the vector path
// (lo > 0: a reduced-resolution decode, which runs the synthesis levels lo .. wl - 1 only)
inline bool dwt_c16_geometry_ok(int aw, int ah, int wl, int lo = 0)
{   // every level on the vector path: level widths multiples of 4 (and rows 16-byte aligned: aw % 4 == 0)
    if (const char *e = getenv("PICSONG_DWT_NOVEC")) if (atoi(e) != 0) return false;
    for (int l = lo; l < wl; l++) {
        const int W = aw >> l;
        if (W < 4 || (W & 3) || ((W >> 1) & 1)) return false;
    }
    return (aw & 3) == 0 && (ah >> (wl - 1)) >= 2;
}
// c16: the coded coefficients at d_in are an int16 Mallat array (the decode frame paths, DwtInvArgs::c16): the vector
// kernels' C16 instantiations on every level, or not at all (the caller looks at plan_inv_is_c16)
inline std::vector<InvLaunch> plan_dwt_inverse(const int32_t *d_in, void *d_out, int aw, int ah, int wl,
                                               float qs, bool fast = false, bool c16 = false)
{
    std::vector<InvLaunch> v;
    int W = aw >> (wl - 1), H = ah >> (wl - 1);
    size_t read_off = 0, write_off = 0;
    for (int l = wl - 1; l >= 0; l--) {
        const bool first = (l == wl - 1);
        InvLaunch f;
        DwtInvArgs &a = f.a;
        a.mallat = d_in; a.AW = aw;
        a.ll = first ? (const void *)d_in : (const void *)((const char *)d_out + read_off * 4);
        a.ll_stride = first ? aw : (W >> 1);
        a.first = first ? 1 : 0;
        a.W = W; a.H = H;
        a.dst = (char *)d_out + write_off * 4;
        a.dst_u8 = nullptr; a.off = 0;
        a.dst_u16 = nullptr; a.px_max = 0;
        a.mallat_z = a.ll_z = a.dst_z = a.u8_z = 0;
        {   // qs = 2^k: dividing by it is exact scaling, dwt_inv97_kernel folds it into the step
            int e = 0;
            a.one_div = std::frexp(qs, &e) == 0.5f ? 1 : 0;
            const char *x = getenv("PICSONG_DWT_EXACT_REPLAY");
            a.exact_replay = x && atoi(x) != 0 ? 1 : 0;
        }
        a.qs = qs;
        a.rqs = 1.0f / qs;
        for (int k = 0; k < 4; k++) { a.q[k] = kQSteps[l][k]; a.rq[k] = 1.0f / a.q[k]; }
        f.fast = fast;
        const int strips = (W + kStripUseful - 1) / kStripUseful;
        f.band = fast ? inv97_band_rows(l, strips, H) : fwd_band_rows(l, strips, H);
        f.gx = (unsigned)((strips + 3) / 4);
        f.gy = (unsigned)(((H >> 1) + f.band / 2 - 1) / (f.band / 2));
        f.vec = dwt_vec_ok(W, aw, d_in, d_out);
        a.c16 = c16 ? 1 : 0;
        v.push_back(f);
        read_off = write_off;
        write_off += (size_t)W * (size_t)H;
        W <<= 1; H <<= 1;
    }
    bool all_vec = true;
    for (const InvLaunch &f : v) all_vec = all_vec && f.vec;
    if (!all_vec) for (InvLaunch &f : v) f.a.c16 = 0;
    return v;
}
inline bool plan_inv_is_c16(const std::vector<InvLaunch> &plan) { return !plan.empty() && plan[0].a.c16 != 0; }

// ---- reduced-quality decode (picsong_ctx_set_decode_drop; no reference counterpart): the planes a codeblock leaves
// undecoded under the context's `drop`.  The level of raster codeblock cb is that of its top-left sample (find_subband,
// bpc_kernels.hpp: 0 the finest detail level, wl the LL band) -- one value a codeblock, also where it straddles subbands --
// and it drops max(0, drop - level) planes: one plane more a level finer, about the growth of a coefficient's weight in
// the image per synthesis level.
constexpr int kDropMax = 15;
inline bool drop_ok(int drop) { return drop >= 0 && drop <= kDropMax; }
inline int codeblock_level(int aw, int ah, int wl, int cb)
{
    const int ncx = aw / 64, x = (cb % ncx) * 64, y = (cb / ncx) * 64;
    for (int a = 1; a <= wl; a++)
        if (x >= (aw >> a) || y >= (ah >> a)) return a - 1;
    return wl;
}
inline int drop_planes_of(int aw, int ah, int wl, int drop, int cb)
{
    const int lv = codeblock_level(aw, ah, wl, cb);
    return drop > lv ? drop - lv : 0;
}

// ---- reduced-resolution decode (picsong_decode_frame_reduced and its mirrors; no reference counterpart).  The image
// at 1/2^r of the frame's size is LL_r, the synthesis stopped after level r.  Its inputs -- the subbands of levels
// r + 1 .. wl and LL_wl -- fill the corner [0, AW >> r) x [0, AH >> r) of the Mallat array, so only the codeblocks that
// meet that corner are decoded: the first ncx_r columns of the first ncy_r codeblock rows.
struct ReducedRect { int ncx_r, ncy_r; };
inline bool reduce_ok(int wl, int r) { return r >= 0 && r <= wl - 1; }
inline ReducedRect reduced_rect(int aw, int ah, int r)
{
    return { ((aw >> r) + 63) / 64, ((ah >> r) + 63) / 64 };
}
// decoder waves of one frame: two codeblocks a wave, the rectangle's codeblocks in row order (BpcArgs::ncx_r)
inline int reduced_waves(const ReducedRect &q) { return (q.ncx_r * q.ncy_r + 1) / 2; }
// picsong_reduced_dims: d = { visible width, height (ceil(W / 2^r) x ceil(H / 2^r)), padded width, height, codeblocks }
inline void reduced_dims(int w, int h, int aw, int ah, int r, int d[5])
{
    const ReducedRect q = reduced_rect(aw, ah, r);
    d[0] = (w + (1 << r) - 1) >> r; d[1] = (h + (1 << r) - 1) >> r;
    d[2] = aw >> r; d[3] = ah >> r;
    d[4] = q.ncx_r * q.ncy_r;
}
// the synthesis levels wl - 1 .. r of plan_dwt_inverse: level r's output, (AW >> r) x (AH >> r) with row stride AW >> r,
// is the reduced image.  The 16-bit form stays where the levels that run all take the vector kernels.
inline std::vector<InvLaunch> plan_dwt_inverse_reduced(const int32_t *d_in, void *d_out, int aw, int ah, int wl, float qs,
                                                       bool fast, bool c16, int r)
{
    std::vector<InvLaunch> v = plan_dwt_inverse(d_in, d_out, aw, ah, wl, qs, fast, c16);
    v.resize(v.size() - (size_t)r);
    bool all_vec = true;
    for (const InvLaunch &f : v) all_vec = all_vec && f.vec;
    for (InvLaunch &f : v) f.a.c16 = c16 && all_vec ? 1 : 0;
    return v;
}

// The Mallat work buffer's elements beyond the frame's P: the LL arrays of levels 1 .. wl - 1 (picsong_dwt_extra)
inline size_t dwt_extra(int aw, int ah, int wl)
{
    size_t e = 0;
    for (int l = 1; l < wl; l++) e += (size_t)(aw >> l) * (size_t)(ah >> l);
    return e;
}

// The frame paths' synthesis plan.  d_pixels != nullptr: the finest level writes clamped u8 pixels there (level shift
// `off` + clamp fused, when its vector kernel applies) instead of T samples into d_out; *fused says so.
// frames > 1 (picsong_decode_frames): grid.z = frame; frame z's coded coefficients at d_in + z * P coefficients, its
// work buffer at d_out + z * (P + extra) elements, its pixels at d_pixels + z * pix_stride bytes.
// want_c16: the decoder may write 16-bit coefficients (picsong_ctx::c16_dec) -- the plan says whether this call's
// pointers allow it (plan_inv_is_c16), BEFORE the decoder is launched: this plan, then the decoder, then run_inverse.
// (the grey frame paths take the 16-bit form only with the fused pixel store; planes_out: an RGB frame's components,
// whose finest level writes T samples for the inverse colour transform, take it too)
// reduce > 0: the levels wl - 1 .. reduce only (plan_dwt_inverse_reduced), level `reduce` the one that writes the pixels
inline std::vector<InvLaunch> plan_inverse_frames(const int32_t *d_in, void *d_out, uint8_t *d_pixels, bool *fused, unsigned frames,
                                                  size_t pix_stride, bool want_c16, bool planes_out, int reduce, int aw, int ah,
                                                  int wl, float qs, bool fast_div, int off, size_t P, size_t extra, int px_max = 0)
{
    if (fused) *fused = false;
    if (px_max > 0) {
        // a deep context: d_pixels holds uint16 samples, pix_stride bytes a frame.  32-bit coefficients; the finest level
        // stores the clamped samples itself (dwt_inv_kernel's U16OUT form) where it is a vector launch, the samples start
        // 16-byte aligned (stride included) and PICSONG_DEEP_NOFUSE is not set
        const bool px16 = d_pixels && (((uintptr_t)d_pixels) & 15u) == 0 && (frames <= 1 || (pix_stride & 15u) == 0) && !deep_nofuse();
        std::vector<InvLaunch> plan = plan_dwt_inverse_reduced(d_in, d_out, aw, ah, wl, qs, fast_div, false, reduce);
        if (px16 && !plan.empty() && plan.back().vec) {
            plan.back().a.dst_u16 = (uint16_t *)d_pixels;
            plan.back().a.off = off;
            plan.back().a.px_max = px_max;
            if (fused) *fused = true;
        }
        if (frames > 1) {
            const unsigned long long wrk_z = (unsigned long long)(P + extra) * 4ull;
            for (InvLaunch &f : plan) {
                f.a.mallat_z = (unsigned long long)P * 4ull;
                f.a.ll_z = f.a.first ? f.a.mallat_z : wrk_z;
                f.a.dst_z = wrk_z;
                f.a.u8_z = (unsigned long long)pix_stride;
            }
        }
        return plan;
    }
    const bool px = d_pixels && (((uintptr_t)d_pixels) & 3u) == 0 && (pix_stride & 3u) == 0;
    std::vector<InvLaunch> plan = plan_dwt_inverse_reduced(d_in, d_out, aw, ah, wl, qs, fast_div, want_c16 && (px || planes_out), reduce);
    if (px && !plan.empty() && plan.back().vec) {
        plan.back().a.dst_u8 = d_pixels;
        plan.back().a.off = off;
        if (fused) *fused = true;
    }
    if (frames > 1) {
        const unsigned long long in_z = (unsigned long long)P * (plan_inv_is_c16(plan) ? 2ull : 4ull);
        const unsigned long long wrk_z = (unsigned long long)(P + extra) * 4ull;
        for (InvLaunch &f : plan) {
            f.a.mallat_z = in_z;
            f.a.ll_z = f.a.first ? in_z : wrk_z;            // the coarsest level's LL comes from the coded array
            f.a.dst_z = wrk_z;
            f.a.u8_z = (unsigned long long)pix_stride;
        }
    }
    return plan;
}

// ---- window decode (picsong_decode_frame_window and its mirrors; no reference counterpart).  The window R_r =
// [x, x + w) x [y, y + h) of the 1/2^r image (LL_r) depends on a cone of the Mallat array.  Per synthesis level
// l = r .. wl - 1 (level l outputs LL_l, W_l x H_l = (AW >> l) x (AH >> l)), the rectangle R_l of LL_l needs the
// rectangle S_l of level l's subband coordinates (W_l / 2 x H_l / 2), per axis, with [a, b) = R_l and K the subband size:
//   5/3: [max(0, floor(a / 2) - 1), min(K, ceil(b / 2) + 1))    9/7: [max(0, floor(a / 2) - 2), min(K, ceil(b / 2) + 2))
// -- the 2 and 4 lifting steps of the synthesis; the symmetric extension at the true edges stays inside the clamped
// interval.  R_{l+1} = S_l.  Level l reads S_l in HL (+W_l / 2 in x), LH (+H_l / 2 in y) and HH (both), and level
// wl - 1 reads S_{wl-1} itself as LL_wl.  The call decodes the 64 x 64 codeblocks of the Mallat raster that meet one of
// those at most 3 (wl - r) + 1 rectangles, each codeblock once.  The whole padded reduced image's window is the reduced
// call's corner (reduced_rect).
struct IRect { int x0, y0, x1, y1; };                   // [x0, x1) x [y0, y1)
constexpr int kWindowMaxRects = 22;                     // 3 (wl - r) + 1, wl <= 7
struct WindowPlan {
    int r, wl, lossy;
    IRect R[8];                                         // R[l], l = r .. wl: LL_l's rectangle (R[r] the window, R[wl] = S[wl - 1])
    IRect S[8];                                         // S[l], l = r .. wl - 1: level l's subband rectangle
    int n_rects;
    IRect cb[kWindowMaxRects];                          // the Mallat rectangles in codeblock units, level wl - 1 first
    int n_cb;                                           // distinct codeblocks among them
    int n_cb_listed;                                    // the rectangles' codeblocks, a codeblock counted once per rectangle
};
inline bool window_ok(int paw, int pah, int x, int y, int w, int h)
{
    return w >= 1 && h >= 1 && x >= 0 && y >= 0 && (long long)x + w <= paw && (long long)y + h <= pah;
}
inline WindowPlan window_plan(int aw, int ah, int wl, bool lossy, int r, int x, int y, int w, int h)
{
    WindowPlan p;
    p.r = r; p.wl = wl; p.lossy = lossy ? 1 : 0;
    const int e = lossy ? 2 : 1;
    auto cone = [e](int a, int b, int K, int &lo, int &hi) {
        lo = a / 2 - e; if (lo < 0) lo = 0;
        hi = (b + 1) / 2 + e; if (hi > K) hi = K;
    };
    p.R[r] = { x, y, x + w, y + h };
    for (int l = r; l < wl; l++) {
        const int hW = (aw >> l) / 2, hH = (ah >> l) / 2;
        IRect s;
        cone(p.R[l].x0, p.R[l].x1, hW, s.x0, s.x1);
        cone(p.R[l].y0, p.R[l].y1, hH, s.y0, s.y1);
        p.S[l] = s; p.R[l + 1] = s;
    }
    p.n_rects = 0;
    auto add = [&p](int x0, int y0, int x1, int y1) { p.cb[p.n_rects++] = { x0 / 64, y0 / 64, (x1 + 63) / 64, (y1 + 63) / 64 }; };
    for (int l = wl - 1; l >= r; l--) {
        const IRect &s = p.S[l];
        const int hW = (aw >> l) / 2, hH = (ah >> l) / 2;
        if (l == wl - 1) add(s.x0, s.y0, s.x1, s.y1);
        add(s.x0 + hW, s.y0, s.x1 + hW, s.y1);
        add(s.x0, s.y0 + hH, s.x1, s.y1 + hH);
        add(s.x0 + hW, s.y0 + hH, s.x1 + hW, s.y1 + hH);
    }
    const int ncx = aw / 64;
    std::vector<uint8_t> seen((size_t)ncx * (size_t)(ah / 64), 0);
    p.n_cb = p.n_cb_listed = 0;
    for (int i = 0; i < p.n_rects; i++) {
        const IRect &q = p.cb[i];
        p.n_cb_listed += (q.x1 - q.x0) * (q.y1 - q.y0);
        for (int cy = q.y0; cy < q.y1; cy++)
            for (int cx = q.x0; cx < q.x1; cx++) {
                uint8_t &v = seen[(size_t)cy * ncx + cx];
                p.n_cb += v ? 0 : 1;
                v = 1;
            }
    }
    return p;
}
// decoder waves of one frame of a window call: two listed codeblocks a wave (a codeblock an earlier rectangle holds
// is listed again and skipped, BpcArgs::win_n)
inline int window_waves(const WindowPlan &p) { return (p.n_cb_listed + 1) / 2; }
// the most waves a window call of the context can need -- the whole image at r = 0 lists every rectangle at its
// largest -- whole workgroups of `wg` waves: what the decoder's plane scratch holds for each frame
inline int window_waves_cap(int aw, int ah, int wl, bool lossy, int ncb, int wg)
{
    int wv = window_waves(window_plan(aw, ah, wl, lossy, 0, 0, 0, aw, ah));
    if (wv < (ncb + 1) / 2) wv = (ncb + 1) / 2;
    return (wv + wg - 1) / wg * wg;
}

// May a decode context take the 16-bit coefficient form between its decoder and its synthesis?  The bound of coef16_ok
// (an honest stream of such a context has no magnitude of 2^15 or more), the vector kernels on every level, at least
// two levels (the coarsest level that also writes pixels has no C16 instantiation), and for 9/7 the verified
// reciprocal divisions (the lean kernels are the ones with a C16 form).  PICSONG_DEC_C16=0 keeps the 32-bit arrays.
// lo > 0: a reduced-resolution decode's synthesis, levels lo .. wl - 1 (the two-level minimum counts those).
inline bool dec_c16_ok(bool lossy, int wl, float qs, int in_max, int aw, int ah, bool fast_div, int lo = 0)
{
    if (const char *e = getenv("PICSONG_DEC_C16")) if (atoi(e) == 0) return false;
    if (const char *e = getenv("PICSONG_DWT_INV97")) if (atoi(e) == 0) return false;
    return wl - lo >= 2 && (!lossy || fast_div) && coef16_ok(lossy, wl, qs, in_max) && dwt_c16_geometry_ok(aw, ah, wl, lo);
}

// Synthesis levels 1 and 0 of an inverse plan as ONE launch of dwt_inv2_kernel (dwt_kernels.hpp): the decode frame
// paths (16-bit coefficients in, pixels out), level 1 not the coarsest, whole 32-row bands.  PICSONG_DWT_NOFUSE_INV=1
// keeps the two launches (the tests cross-check both).
struct Inv2Launch { DwtInv2Args a; unsigned gx, gy; };
inline bool plan_dwt_inv2(const std::vector<InvLaunch> &plan, Inv2Launch &f, bool lossy)
{
    if (const char *e = getenv("PICSONG_DWT_NOFUSE_INV")) if (atoi(e) != 0) return false;
    if (plan.size() < 3) return false;
    const InvLaunch &p1 = plan[plan.size() - 2], &p0 = plan.back();
    if (!p0.vec || !p1.vec || !p0.a.c16 || !p0.a.dst_u8 || p1.a.first) return false;
    // 9/7: built, bit-identical and NOT the default -- the 9/7 synthesis is bound by its arithmetic (three-instruction
    // divisions the reference's rounding demands), not by traffic, and the fused form pays for the LL0 bytes it saves
    // with level 1's longer run-in (14 steps for 8 row pairs) and 128 registers (4 waves a SIMD): an 8K frame's
    // levels 1 + 0 take 48.0 us fused against 15.3 + 35.1 us, decode with three calls in flight 150 against 157
    // Gpixel/s (round 4, profiles/NOTES.md).  PICSONG_DWT_FUSE_INV97=1 selects it (the tests run both).
    if (lossy) {
        const char *e = getenv("PICSONG_DWT_FUSE_INV97");
        if (!(e && atoi(e) != 0) || !p0.fast) return false;
    }
    if (p0.a.W < 16 || (p0.a.W & 7) || p0.a.H < 64 || (p0.a.H % (4 * kI2Pairs))) return false;
    f.a.l1 = p1.a; f.a.l0 = p0.a;
    const int useful = lossy ? i2_useful<true>() : i2_useful<false>();
    const int strips = (p0.a.W + useful - 1) / useful;
    f.gx = (unsigned)((strips + 3) / 4);
    f.gy = (unsigned)(p0.a.H / (4 * kI2Pairs));
    return true;
}

}  // namespace picsong
