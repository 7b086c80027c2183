// kernel_select.hpp -- which template instantiation of a kernel a planned launch takes, with its grid and its scratch
// (pure host code, no device code: functions from a plan's fields or a coder's mode flags to a kernel function pointer).
// The one copy of that policy.  Its callers are the launch sequences of launch_seq.hpp, which the C-ABI implementation
// (picsong_hip.hip) and the CPU wave-emulator drivers (tests/hipemu/) both run, each through its own launcher; a single
// launch whose arguments come from a helper here (select_stats / stats_args, select_quantise / quantise_args) goes
// through that launcher directly.
// What the environment says arrives as a parameter (lean97, the coders' `compact`): each caller reads its switches at
// the moment it always did.
#pragma once
#include <string.h>

#include "bpc_kernels.hpp"
#include "dwt_kernels.hpp"
#include "launch_plan.hpp"
#include "layout_kernels.hpp"
#include "pack_kernels.hpp"
#include "quality_kernels.hpp"
#include "rate_kernels.hpp"
#include "rate_search.hpp"
#include "train_kernels.hpp"
#include "window_kernels.hpp"

namespace picsong {

using FwdKernel = void (*)(DwtFwdArgs);
using Fwd2Kernel = void (*)(DwtFwd2Args);
using InvKernel = void (*)(DwtInvArgs);
using Inv2Kernel = void (*)(DwtInv2Args);
using InvRgbKernel = void (*)(DwtInvArgs, uint8_t *, uint8_t *, uint8_t *);
using WinKernel = void (*)(WinSynArgs);
using BpcKernel = void (*)(BpcArgs);
using StatsKernel = void (*)(BpcArgs, unsigned long long *, int);
using QuantKernel = void (*)(QuantArgs);
using SseKernel = void (*)(SseArgs);
using LayoutKernel = void (*)(LayoutArgs);

// ---- forward transform: one level (256 threads, grid f.gx x f.gy x frames)
template <int BAND, bool VEC>
inline FwdKernel fwd_kernel_of(bool lossy, bool u8)
{
    if (lossy) return u8 ? dwt_fwd_kernel<float, true, true, BAND, VEC> : dwt_fwd_kernel<float, true, false, BAND, VEC>;
    return u8 ? dwt_fwd_kernel<int, false, true, BAND, VEC> : dwt_fwd_kernel<int, false, false, BAND, VEC>;
}
// a deep context's level 0 (FwdLaunch::u16): the uint16 load stage
template <int BAND, bool VEC>
inline FwdKernel fwd16_kernel_of(bool lossy)
{
    return lossy ? dwt_fwd_kernel<float, true, false, BAND, VEC, true> : dwt_fwd_kernel<int, false, false, BAND, VEC, true>;
}
inline FwdKernel select_fwd16(bool lossy, const FwdLaunch &f)
{
    switch (f.band) {
    case 32: return f.vec ? fwd16_kernel_of<32, true>(lossy) : fwd16_kernel_of<32, false>(lossy);
    case 16: return f.vec ? fwd16_kernel_of<16, true>(lossy) : fwd16_kernel_of<16, false>(lossy);
    case 8: return f.vec ? fwd16_kernel_of<8, true>(lossy) : fwd16_kernel_of<8, false>(lossy);
    default: return f.vec ? fwd16_kernel_of<4, true>(lossy) : fwd16_kernel_of<4, false>(lossy);
    }
}
// a deep RGB context's level 0 (FwdLaunch::rgb16): the three planes' uint16 load stage with the colour transform; the
// per-column form in bands of at most kRgb16ColumnMaxBand rows (plan_dwt_forward_rgb16 gives it no taller one)
template <int BAND, bool VEC>
inline FwdKernel fwd_rgb16_kernel_of(bool lossy)
{
    return lossy ? dwt_fwd_kernel<float, true, false, BAND, VEC, false, true> : dwt_fwd_kernel<int, false, false, BAND, VEC, false, true>;
}
inline FwdKernel select_fwd_rgb16(bool lossy, const FwdLaunch &f)
{
    static_assert(kRgb16ColumnMaxBand == 8, "the per-column instantiations below");
    switch (f.band) {
    case 32: return f.vec ? fwd_rgb16_kernel_of<32, true>(lossy) : fwd_rgb16_kernel_of<8, false>(lossy);
    case 16: return f.vec ? fwd_rgb16_kernel_of<16, true>(lossy) : fwd_rgb16_kernel_of<8, false>(lossy);
    case 8: return f.vec ? fwd_rgb16_kernel_of<8, true>(lossy) : fwd_rgb16_kernel_of<8, false>(lossy);
    default: return f.vec ? fwd_rgb16_kernel_of<4, true>(lossy) : fwd_rgb16_kernel_of<4, false>(lossy);
    }
}
inline FwdKernel select_fwd(bool lossy, const FwdLaunch &f)
{
    if (f.rgb16) return select_fwd_rgb16(lossy, f);
    if (f.u16) return select_fwd16(lossy, f);
    switch (f.band) {
    case 32: return f.vec ? fwd_kernel_of<32, true>(lossy, f.u8) : fwd_kernel_of<32, false>(lossy, f.u8);
    case 16: return f.vec ? fwd_kernel_of<16, true>(lossy, f.u8) : fwd_kernel_of<16, false>(lossy, f.u8);
    case 8: return f.vec ? fwd_kernel_of<8, true>(lossy, f.u8) : fwd_kernel_of<8, false>(lossy, f.u8);
    default: return f.vec ? fwd_kernel_of<4, true>(lossy, f.u8) : fwd_kernel_of<4, false>(lossy, f.u8);
    }
}

// ---- the fused forward head, levels 0 and 1 (256 threads, grid f2.gx x f2.gy x frames)
// c16: coded subbands as int16 (DwtFwdArgs::c16); rgb: the colour transform in the load stage, grid.z = component
// (RCT on the integer head, ICT on the 9/7 one; plan_dwt_fwd2 with kF2PairsRgb, always 16-bit)
// nb: the plan's nb_override (f2_pairs_batched: the 5/3 int16 head's longer bands for calls of several frames)
inline Fwd2Kernel select_fwd2(bool lossy, bool c16, bool rgb = false, int nb = 0)
{
    if (nb == kF2PairsBatch && !lossy && c16 && !rgb) return dwt_fwd2_kernel<int, false, true, kF2PairsBatch, true>;
    if (rgb) return lossy ? dwt_fwd2_kernel<float, true, true, kF2PairsRgb, true, true> : dwt_fwd2_kernel<int, false, true, kF2PairsRgb, true, true>;
    if (c16) return lossy ? dwt_fwd2_kernel<float, true, true, kF2PairsLossy, true> : dwt_fwd2_kernel<int, false, true, kF2Pairs, true>;
    return lossy ? dwt_fwd2_kernel<float, true, true, kF2PairsLossy> : dwt_fwd2_kernel<int, false, true, kF2Pairs>;
}

// the rate calls' RGB head (plan_dwt_forward_unit): the ICT in the load stage, the coefficients in the 32-bit float form
inline Fwd2Kernel select_fwd2_rgb_f32() { return dwt_fwd2_kernel<float, true, true, kF2PairsRgb, false, true>; }

// ---- synthesis: one level (256 threads, grid f.gx x f.gy x frames)
template <int BAND, bool C16>
inline InvKernel inv97_kernel_of(const DwtInvArgs &a)
{
    if (a.dst_u8) return a.one_div ? dwt_inv97_kernel<BAND, true, false, true, C16> : dwt_inv97_kernel<BAND, true, false, false, C16>;
    if (a.first) return a.one_div ? dwt_inv97_kernel<BAND, false, true, true, C16> : dwt_inv97_kernel<BAND, false, true, false, C16>;
    return a.one_div ? dwt_inv97_kernel<BAND, false, false, true, C16> : dwt_inv97_kernel<BAND, false, false, false, C16>;
}
template <int BAND, bool VEC, bool U8OUT>
inline InvKernel inv_kernel_of(bool lossy, bool fast)
{
    if (lossy && fast) return dwt_inv_kernel<float, true, BAND, VEC, U8OUT, true>;
    if (lossy) return dwt_inv_kernel<float, true, BAND, VEC, U8OUT>;
    return dwt_inv_kernel<int, false, BAND, VEC, U8OUT>;
}
// a deep context's finest level (DwtInvArgs::dst_u16; a vector launch with 32-bit coefficients, plan_inverse_frames): the
// uint16 store -- 5/3, 9/7 dividing and 9/7 FAST; never the lean kernel, which has no such form
template <int BAND>
inline InvKernel inv16_kernel_of(bool lossy, bool fast)
{
    if (lossy && fast) return dwt_inv_kernel<float, true, BAND, true, false, true, false, true>;
    if (lossy) return dwt_inv_kernel<float, true, BAND, true, false, false, false, true>;
    return dwt_inv_kernel<int, false, BAND, true, false, false, false, true>;
}
template <int BAND>
inline InvKernel inv_level_of(bool lossy, bool lean97, const InvLaunch &f)
{
    if (f.a.dst_u16) return inv16_kernel_of<BAND>(lossy, f.fast);
    if (f.a.c16) {
        // the decode frame paths' 16-bit coefficients (dec_c16_ok: vector kernels, 9/7 through the lean kernel, the
        // coarsest level never the one that writes pixels)
        if (lossy) return inv97_kernel_of<BAND, true>(f.a);
        return f.a.dst_u8 ? dwt_inv_kernel<int, false, BAND, true, true, false, true> : dwt_inv_kernel<int, false, BAND, true, false, false, true>;
    }
    // f.fast: the 9/7 divisions in their reciprocal form (verified for the context's qs at creation); the vector
    // launches of such a context are the lean kernel's (lean97 = false, PICSONG_DWT_INV97=0: dwt_inv_kernel's FAST
    // instantiations)
    // (a coarsest level that also writes pixels, wl = 1, stays with dwt_inv_kernel)
    if (lossy && f.fast && lean97 && f.vec && !(f.a.first && f.a.dst_u8)) return inv97_kernel_of<BAND, false>(f.a);
    if (f.vec && f.a.dst_u8) return inv_kernel_of<BAND, true, true>(lossy, f.fast);   // finest level of the frame path: pixels out, clamp fused
    return f.vec ? inv_kernel_of<BAND, true, false>(lossy, f.fast) : inv_kernel_of<BAND, false, false>(lossy, f.fast);
}
inline InvKernel select_inv(bool lossy, bool lean97, const InvLaunch &f)
{
    switch (f.band) {
    case 32: return inv_level_of<32>(lossy, lean97, f);
    case 16: return inv_level_of<16>(lossy, lean97, f);
    case 8: return inv_level_of<8>(lossy, lean97, f);
    default: return inv_level_of<4>(lossy, lean97, f);
    }
}

// ---- the fused synthesis pair, levels 1 and 0 (plan_dwt_inv2; 256 threads, grid f2.gx x f2.gy x frames)
inline Inv2Kernel select_inv2(bool lossy, bool one_div)
{
    if (!lossy) return dwt_inv2_kernel<false, false>;
    return one_div ? dwt_inv2_kernel<true, true> : dwt_inv2_kernel<true, false>;
}

// ---- the fused RGB synthesis tails: the finest level of the three components + the inverse colour transform as one
// launch.  5/3: dwt_inv_rgb_kernel on the level's own grid; 9/7: dwt_inv97_rgb_kernel, the components as the three
// waves of a workgroup, one strip a workgroup.
struct InvRgbLaunch { InvRgbKernel kernel; unsigned gx, gy, threads; };
inline InvRgbLaunch select_inv_rgb(bool lossy, const InvLaunch &f)
{
    if (!lossy) {
        switch (f.band) {
        case 32: return { dwt_inv_rgb_kernel<32>, f.gx, f.gy, 256 };
        case 16: return { dwt_inv_rgb_kernel<16>, f.gx, f.gy, 256 };
        case 8: return { dwt_inv_rgb_kernel<8>, f.gx, f.gy, 256 };
        default: return { dwt_inv_rgb_kernel<4>, f.gx, f.gy, 256 };
        }
    }
    const unsigned gx = (unsigned)((f.a.W + kStripUseful - 1) / kStripUseful);
    switch (f.band) {
    case 32: return { f.a.one_div ? dwt_inv97_rgb_kernel<32, true> : dwt_inv97_rgb_kernel<32, false>, gx, f.gy, 192 };
    case 16: return { f.a.one_div ? dwt_inv97_rgb_kernel<16, true> : dwt_inv97_rgb_kernel<16, false>, gx, f.gy, 192 };
    case 8: return { f.a.one_div ? dwt_inv97_rgb_kernel<8, true> : dwt_inv97_rgb_kernel<8, false>, gx, f.gy, 192 };
    default: return { f.a.one_div ? dwt_inv97_rgb_kernel<4, true> : dwt_inv97_rgb_kernel<4, false>, gx, f.gy, 192 };
    }
}

// ---- the window synthesis (256 threads, the WinLaunch's grid)
inline WinKernel select_window(bool lossy, bool u8)
{
    if (lossy) return u8 ? dwt_window_kernel<float, kWinOutU8> : dwt_window_kernel<float, kWinOutT>;
    return u8 ? dwt_window_kernel<int, kWinOutU8> : dwt_window_kernel<int, kWinOutT>;
}
// ... by a launch's output form (WinLaunch::out): kWinOutU16 is level r of a deep grey call
inline WinKernel select_window_out(bool lossy, int out)
{
    if (out != kWinOutU16) return select_window(lossy, out == kWinOutU8);
    return lossy ? dwt_window_kernel<float, kWinOutU16> : dwt_window_kernel<int, kWinOutU16>;
}

// ---- the coders: kernel, threads a workgroup, workgroups for `waves` waves (a wave codes a codeblock pair), and the
// dwords of BpcArgs::plane_scratch the launch needs (whole workgroups)
struct BpcLaunch { BpcKernel kernel; unsigned threads, wgs; size_t scratch_dwords; };
inline BpcLaunch bpc_launch(BpcKernel kernel, int wg_waves, unsigned waves)
{
    const unsigned wgs = (waves + (unsigned)wg_waves - 1) / (unsigned)wg_waves;
    return { kernel, 64u * (unsigned)wg_waves, wgs, (size_t)wgs * (size_t)wg_waves * kEncScratchDwordsPerWave };
}
// cp3: three coding passes, one kernel for both directions (bpc3_kernel).  bulk (-k > 0): the BULK instantiation (bulk
// scan below the consecutive bit-planes, tables in LDS), one-wave workgroups.
// Two instantiations of the -k > 0 encoder: with compact table copies it is asked for six waves a SIMD (80
// registers, some of its prologue spilled) -- what frames in flight want: 133 -> 142 Gpixel/s at k = 0.5; with
// whole tables its LDS bounds it to four waves anyway, it takes 102 registers and spills nothing -- what a lone
// frame wants, whose 4080 waves are four to a SIMD whatever the kernel allows: 0.376 against 0.411 ms.  The
// context's hint (picsong_ctx_set_pipelined) chooses: compact_pipelined = the tables fit the compact copies
// (bulk_compact) and the hint is set.
inline BpcLaunch select_encoder(bool cp3, bool bulk, bool compact_pipelined, unsigned waves)
{
    if (cp3) return bpc_launch(bpc3_kernel<false>, kBpc3WgWaves, waves);
    if (bulk) return bpc_launch(compact_pipelined ? bpc_encode_kernel<true, true> : bpc_encode_kernel<true>, 1, waves);
    return bpc_launch(bpc_encode_kernel<false>, kBpcEncWgWaves, waves);
}
// compact (-k > 0): the COMPACT table copies (bulk_compact); from_stream: the codewords come from the packed stream
// (BpcArgs::cw16*), not the staging; c16 (with from_stream only): the coefficients leave as an int16 Mallat array.
// kernel = nullptr: refused -- the 16-bit coefficient form decodes from the stream itself.
// (-k > 0 is one launch: the two-pass planes are parked in the scratch whatever their number)
// drop (BpcArgs::drop > 0, k = 0 and -cp 2 only -- refused elsewhere): the reduced-quality kernels, one for each of the
// three k = 0 forms, on the same grid and scratch; false: exactly the choice below, as ever
inline BpcLaunch select_decoder(bool cp3, bool bulk, bool compact, bool from_stream, bool c16, unsigned waves, bool drop = false)
{
    if (c16 && !from_stream) return { nullptr, 0, 0, 0 };
    if (drop) {
        if (cp3 || bulk) return { nullptr, 0, 0, 0 };
        if (c16) return bpc_launch(bpc_decode_drop_kernel<true, true>, kBpcDecWgWaves, waves);
        if (from_stream) return bpc_launch(bpc_decode_drop_kernel<true>, kBpcDecWgWaves, waves);
        return bpc_launch(bpc_decode_drop_kernel<>, kBpcDecWgWaves, waves);
    }
    if (cp3) return bpc_launch(bpc3_kernel<true>, kBpc3WgWaves, waves);
    if (bulk) {
        BpcKernel k = compact ? bpc_decode_kernel<true, kDecSmallPlanes, false, false, true> : bpc_decode_kernel<true, kDecSmallPlanes>;
        if (c16) k = compact ? bpc_decode_kernel<true, kDecSmallPlanes, true, true, true> : bpc_decode_kernel<true, kDecSmallPlanes, true, true>;
        else if (from_stream) k = compact ? bpc_decode_kernel<true, kDecSmallPlanes, true, false, true> : bpc_decode_kernel<true, kDecSmallPlanes, true>;
        return bpc_launch(k, 1, waves);
    }
    if (c16) return bpc_launch(bpc_decode_kernel<false, kDecSmallPlanes, true, true>, kBpcDecWgWaves, waves);
    if (from_stream) return bpc_launch(bpc_decode_kernel<false, kDecSmallPlanes, true>, kBpcDecWgWaves, waves);
    return bpc_launch(bpc_decode_kernel<false, kDecSmallPlanes>, kBpcDecWgWaves, waves);
}
// The planes of an RGB launch (component z % 3 of frame z / 3, table z % 3): a plane's waves_per_frame for wpf codeblock
// pairs -- k = 0: whole workgroups, so that a workgroup (its LDS table copy) never spans two planes; -k > 0 (one-wave
// workgroups): exactly its waves.
inline int rgb_component_waves(bool bulk, int wpf)
{
    static_assert(kBpcEncWgWaves == kBpcDecWgWaves, "one layout serves the launches of both directions");
    return bulk ? wpf : (wpf + kBpcEncWgWaves - 1) / kBpcEncWgWaves * kBpcEncWgWaves;
}
// the dwords of plane scratch a coder launch of `waves` waves needs (what a caller sizes BpcArgs::plane_scratch by)
inline size_t encoder_scratch_dwords(bool cp3, bool bulk, unsigned waves) { return select_encoder(cp3, bulk, false, waves).scratch_dwords; }
inline size_t decoder_scratch_dwords(bool cp3, bool bulk, unsigned waves) { return select_decoder(cp3, bulk, false, false, false, waves).scratch_dwords; }

// ---- helpers of both sides
// geo: the nine fields in LutGeo's order (the emulator's entry points take them so)
inline LutGeo lut_geo(int nBp, int nSub, int cRef, int cSign, int cSig, int prec, int nRef, int nSig, int nSign)
{
    return LutGeo{ nBp, nSub, cRef, cSign, cSig, prec, nRef, nSig, nSign };
}
inline LutGeo lut_geo(const int *geo) { return lut_geo(geo[0], geo[1], geo[2], geo[3], geo[4], geo[5], geo[6], geo[7], geo[8]); }

// the base BpcArgs of a frame: geometry, table, flag; everything else 0
inline BpcArgs bpc_frame_args(int aw, int ah, int wl, const int32_t *lut, const LutGeo &g, int *range_flag)
{
    BpcArgs a;
    memset(&a, 0, sizeof a);
    a.AW = aw; a.AH = ah; a.wl = wl; a.ncx = aw / 64; a.nCB = (aw / 64) * (ah / 64);
    a.lut = lut; a.g = g; a.range_flag = range_flag;
    return a;
}

// ---- the training statistics (bpc_stats_kernel): a persistent grid over `pairs` codeblock pairs (all frames of the
// call), a wave a pair at a time; the dwords of BpcArgs::plane_scratch its waves need
struct StatsLaunch { StatsKernel kernel; unsigned threads, wgs; size_t scratch_dwords; };
inline unsigned stats_wgs(size_t pairs)
{
    const size_t w = (pairs + kTrainWgWaves - 1) / kTrainWgWaves;
    return (unsigned)(w < 1 ? 1 : (w > kTrainMaxWgs ? kTrainMaxWgs : w));
}
inline StatsLaunch select_stats(size_t pairs)
{
    const unsigned wgs = stats_wgs(pairs);
    return { bpc_stats_kernel, 64u * (unsigned)kTrainWgWaves, wgs, (size_t)wgs * kTrainWgWaves * kEncScratchDwordsPerWave };
}
// the encoder-side arguments of a statistics launch over `frames` coefficient arrays coef_z bytes apart
inline BpcArgs stats_args(int aw, int ah, int wl, const LutGeo &g, int *range_flag, const void *coeffs, bool is_float, bool c16,
                          int frames, unsigned long long coef_z, uint32_t *plane_scratch)
{
    BpcArgs a = bpc_frame_args(aw, ah, wl, nullptr, g, range_flag);
    a.coeffs_in = coeffs; a.is_float = is_float ? 1 : 0; a.c16 = c16 ? 1 : 0;
    a.frames = frames; a.waves_per_frame = (a.nCB + 1) / 2; a.coef_z = coef_z;
    a.plane_scratch = plane_scratch;
    return a;
}
// section sizes a geometry implies for `wl` (IO/IOManager.ipp:431-433) where the caller left them 0
inline void lut_geo_sections(LutGeo &g, int wl)
{
    if (g.nRef <= 0) g.nRef = g.nSub * g.nBp * g.cRef * wl + g.nBp * g.cRef;
    if (g.nSig <= 0) g.nSig = g.nSub * g.nBp * g.cSig * wl + g.nBp * g.cSig;
    if (g.nSign <= 0) g.nSign = g.nSub * g.nBp * g.cSign * wl + g.nBp * g.cSign;
}

// -k > 0: does the table geometry let every codeblock of the frame use the COMPACT LDS copies (bulk_max_span_bytes: the
// geometry's widest codeblock)?  (PICSONG_BULK_FULLTAB=1 keeps the whole-table instantiations: the callers' switch)
inline bool bulk_compact(int aw, int ah, int wl, const LutGeo &g)
{
    return bulk_max_span_bytes(aw, ah, wl, g.nBp, g.nSub, g.cRef, g.cSig, g.cSign) <= kBulkCompactBytes;
}

// ---- the rate calls' quantisation pass (quantise_kernel, rate_kernels.hpp): K = 1..3 candidate gains over the
// unquantised float arrays of n frames, a workgroup (256 threads) a row at a time
struct QuantLaunch { QuantKernel kernel; unsigned wgs; };
// i32 (the quality calls' probes): the int32 form, one candidate a launch
inline QuantLaunch select_quantise(int K, int n, int ah, bool i32 = false)
{
    const size_t rows = (size_t)n * (size_t)ah;
    const unsigned wgs = (unsigned)(rows > 8192 ? 8192 : rows);
    if (i32) return { quantise_kernel<1, true>, wgs };
    return { K >= 3 ? quantise_kernel<3> : (K == 2 ? quantise_kernel<2> : quantise_kernel<1>), wgs };
}
// its arguments: the gains q(j) of `js`, candidate c as int16 where c16[c]; frames src_z / dst_z bytes apart
inline QuantArgs quantise_args(const void *src, unsigned long long src_z, void *dst, unsigned long long dst_z, int aw, int ah,
                               int wl, int n, int K, const int *js, const bool *c16)
{
    QuantArgs a;
    memset(&a, 0, sizeof a);
    a.src = src; a.src_z = src_z; a.dst = dst; a.dst_z = dst_z;
    a.AW = aw; a.AH = ah; a.wl = wl; a.n = n;
    for (int c = 0; c < kQuantMaxK; c++) {
        a.qs[c] = rate_q(js[c < K ? c : K - 1]);
        a.c16[c] = c16[c < K ? c : K - 1] ? 1 : 0;
    }
    for (int l = 0; l < 10; l++)
        for (int k = 0; k < 4; k++) a.q[l][k] = kQSteps[l][k];
    return a;
}

// ---- the distortion measurement (sse_kernel, quality_kernels.hpp): the visible w x h samples of n pairs of padded
// arrays, 256 threads, a tile of 256 * kSseTileLoads vectors a workgroup and step, grid-stride beyond kSseMaxWgs.
// The vector form where both sides' pointers, pitches and strides are 16-byte aligned, else the per-byte one.
struct SseLaunch { SseKernel kernel; unsigned wgs; };
inline SseArgs sse_args(const uint8_t *a, size_t a_pitch, unsigned long long a_z, const uint8_t *b, size_t b_pitch,
                        unsigned long long b_z, int w, int h, int n, unsigned long long *out)
{
    SseArgs s;
    memset(&s, 0, sizeof s);
    s.a = a; s.a_z = a_z; s.a_pitch = (uint32_t)a_pitch;
    s.b = b; s.b_z = b_z; s.b_pitch = (uint32_t)b_pitch;
    s.out = out; s.W = w; s.H = h; s.n = n;
    return s;
}
inline SseLaunch select_sse(const SseArgs &s)
{
    const bool vec = ((((uintptr_t)s.a) | ((uintptr_t)s.b) | s.a_z | s.b_z | s.a_pitch | s.b_pitch) & 15u) == 0;
    const size_t items = (size_t)((s.W + 15) / 16) * (size_t)s.H, tile = 256u * (size_t)kSseTileLoads;
    const size_t tiles = (items + tile - 1) / tile * (size_t)s.n;
    const unsigned wgs = (unsigned)(tiles > kSseMaxWgs ? kSseMaxWgs : (tiles < 1 ? 1 : tiles));
    return { vec ? sse_kernel<true> : sse_kernel<false>, wgs };
}
// ---- the structural measure (ssim_kernel, quality_kernels.hpp) over sse_args' arguments (w, h >= 8: the callers
// refuse less): 256 threads, a tile of four (strip, band) wave items a workgroup and step, grid-stride beyond kSseMaxWgs.
// The dword form where both sides' pointers, pitches and strides are 4-byte aligned, else the per-byte one.
inline bool ssim_geometry_ok(int w, int h) { return w >= 8 && h >= 8; }
inline unsigned long long ssim_windows(int w, int h)
{
    return (unsigned long long)((w - 8) / 4 + 1) * (unsigned long long)((h - 8) / 4 + 1);
}
inline SseLaunch select_ssim(const SseArgs &s)
{
    const bool vec = ((((uintptr_t)s.a) | ((uintptr_t)s.b) | s.a_z | s.b_z | s.a_pitch | s.b_pitch) & 3u) == 0;
    const size_t nx = (size_t)((s.W - 8) / 4 + 1), ny = (size_t)((s.H - 8) / 4 + 1);
    const size_t items = ((nx + kSsimStripWindows - 1) / kSsimStripWindows) * ((ny + kSsimBandWindows - 1) / kSsimBandWindows);
    const size_t tiles = (items + 3) / 4 * (size_t)s.n;
    const unsigned wgs = (unsigned)(tiles > kSseMaxWgs ? kSseMaxWgs : (tiles < 1 ? 1 : tiles));
    return { vec ? ssim_kernel<true> : ssim_kernel<false>, wgs };
}
// ---- the tail of an RGB quality probe (rgb_sse_kernel, quality_kernels.hpp): the inverse ICT of n frames' float
// component planes (plane 3 f + k at c + (3 f + k) * c_z bytes, row pitch c_pitch floats) and the SSE of the visible
// w x h samples against the input planes (frame f's in_z bytes after r / g / b, row pitch in_pitch) in one launch,
// 256 threads, a tile of 256 * kRgbSseTileLoads groups of four pixels a workgroup and step, grid-stride beyond kSseMaxWgs.
// kernel == nullptr: the arguments do not allow its loads (dwordx4 of the floats: c, c_z and the row pitch 16-byte
// aligned; a dword of each input plane: r, g, b, in_z and in_pitch 4-byte aligned), or the caller's switch is off
// (fused = false: PICSONG_RGB_SSE_FUSED=0) -- the caller runs rgb_inverse + frames_sse instead.
using RgbSseKernel = void (*)(RgbSseArgs);
struct RgbSseLaunch { RgbSseKernel kernel; unsigned wgs; };
inline RgbSseArgs rgb_sse_args(const void *c, unsigned long long c_z, size_t c_pitch, const uint8_t *r, const uint8_t *g, const uint8_t *b,
                               unsigned long long in_z, size_t in_pitch, int w, int h, int n, int off, unsigned long long *out)
{
    RgbSseArgs s;
    memset(&s, 0, sizeof s);
    s.c = (const float *)c; s.c_z = c_z; s.c_pitch = (uint32_t)c_pitch;
    s.r = r; s.g = g; s.b = b; s.in_z = n > 1 ? in_z : 0; s.in_pitch = (uint32_t)in_pitch;
    s.out = out; s.W = w; s.H = h; s.n = n; s.off = off;
    return s;
}
inline RgbSseLaunch select_rgb_sse(const RgbSseArgs &s, bool fused = true)
{
    const bool c_ok = ((((uintptr_t)s.c) | s.c_z | ((unsigned long long)s.c_pitch * 4ull)) & 15u) == 0;
    const bool in_ok = ((((uintptr_t)s.r) | ((uintptr_t)s.g) | ((uintptr_t)s.b) | s.in_z | s.in_pitch) & 3u) == 0;
    const bool fits = s.W >= 1 && s.H >= 1 && s.n >= 1 && (size_t)s.W <= s.c_pitch && (size_t)s.W <= s.in_pitch;
    if (!fused || !c_ok || !in_ok || !fits) return { nullptr, 0u };
    const size_t items = (size_t)((s.W + 3) / 4) * (size_t)s.H, tile = 256u * (size_t)kRgbSseTileLoads;
    const size_t tiles = (items + tile - 1) / tile * (size_t)s.n;
    return { rgb_sse_kernel<kRgbSseRunLoads>, (unsigned)(tiles > kSseMaxWgs ? kSseMaxWgs : tiles) };
}

// ---- pixel layouts (ingest_kernel / emit_kernel, layout_kernels.hpp).  bytes a pixel, planes of the padded side
inline bool layout_is_rgb16(int layout) { return layout == kLayoutPlanar3_16 || layout == kLayoutRgb48 || layout == kLayoutRgba64; }
inline int layout_bpp(int layout)
{
    if (layout_is_rgb16(layout)) return layout == kLayoutPlanar3_16 ? 2 : (layout == kLayoutRgb48 ? 6 : 8);
    return layout == kLayoutGrey16 ? 2 : (layout < kLayoutRgb24 ? 1 : (layout < kLayoutRgba32 ? 3 : 4));
}
inline int layout_planes(int layout) { return layout == kLayoutGrey8 || layout == kLayoutGrey16 ? 1 : 3; }
// What picsong_ingest_frames / picsong_emit_frames (and the whole-frame calls over them) refuse, as a message; nullptr:
// the arguments are fine.  `data`, pitch, plane_stride: the picsong_image's; n frames frame_stride bytes apart; the
// padded side at `padded`, frames padded_stride apart.
// deep (a context of 9- to 16-bit samples): GREY16 and nothing else -- or, deep_rgb, PLANAR3_16, RGB48 and RGBA64 and nothing
// else; both false: the six 8-bit layouts, as ever
inline const char *layout_refusal(int layout, const void *data, size_t pitch, size_t plane_stride, size_t frame_stride,
                                  const void *padded, size_t padded_stride, int n, int W, int H, int AW, int AH, bool deep = false,
                                  bool deep_rgb = false)
{
    if (!data || !padded) return "null pointer";
    if (deep_rgb && !layout_is_rgb16(layout)) return "the layouts of a deep RGB context (bit_depth 9..16) are PLANAR3_16, RGB48 and RGBA64";
    if (deep && !deep_rgb && layout != kLayoutGrey16) return "the layout of a deep context (bit_depth 9..16) is GREY16";
    if (!deep && (layout < 0 || layout >= kLayoutCount)) return "unknown layout";
    if (n < 1 || n > kLayoutMaxFrames) return "n outside 1..64";
    if (W < 1 || H < 1 || AW < W || AH < H) return "bad geometry";
    if (AW - W > W || AH - H > H) return "the mirror padding adds more columns / rows than the frame has";
    const size_t row = (size_t)W * (size_t)layout_bpp(layout);
    if (pitch < row) return "pitch smaller than a row of pixels";
    size_t span = (size_t)(H - 1) * pitch + row;                        // the bytes one plane (one interleaved frame) spans
    if (layout == kLayoutPlanar3 || layout == kLayoutPlanar3_16) {
        if (plane_stride < span) return "plane_stride smaller than a plane";
        span += 2 * plane_stride;
    }
    if (n > 1 && frame_stride < span) return "frame_stride smaller than a frame";
    if (layout_is_rgb16(layout)) {
        // (the padded side: three uint16 planes a frame, its stride in bytes)
        if ((((uintptr_t)data) | pitch | (uintptr_t)padded) & 1u) return "16-bit samples need 2-byte aligned pointers and pitch";
        if (layout == kLayoutPlanar3_16 && (plane_stride & 1u)) return "16-bit samples need an even plane_stride";
        if (n > 1 && ((frame_stride | padded_stride) & 1u)) return "16-bit samples need even strides";
        if (n > 1 && padded_stride < 6 * (size_t)AW * (size_t)AH) return "padded_stride smaller than a frame's padded planes";
        return nullptr;
    }
    if (layout == kLayoutGrey16) {
        // (the padded side: uint16 planes, its stride in bytes)
        if ((((uintptr_t)data) | pitch | (uintptr_t)padded) & 1u) return "16-bit samples need 2-byte aligned pointers and pitch";
        if (n > 1 && ((frame_stride | padded_stride) & 1u)) return "16-bit samples need even strides";
        if (n > 1 && padded_stride < 2 * (size_t)AW * (size_t)AH) return "padded_stride smaller than a frame's padded planes";
        return nullptr;
    }
    if (n > 1 && padded_stride < (size_t)layout_planes(layout) * (size_t)AW * (size_t)AH) return "padded_stride smaller than a frame's padded planes";
    return nullptr;
}
// What picsong_encode_rgb_frames / picsong_decode_rgb_frames refuse, as a message; nullptr: the arguments are fine.
// n RGB frames a call, 3 n planes a launch (the batched grid takes 64): r / g / b frame 0's padded planes of P bytes,
// frame f's frame_stride bytes after them; the streams stream_stride shorts apart, a worst-case one max_stream shorts.
// same_geometry: the three component tables agree in geometry (the coder launch has one LutGeo).
constexpr int kRgbMaxFrames = 21;
inline const char *rgb_frames_refusal(bool ctx_rgb, int cp, bool same_geometry, int n, const void *r, const void *g, const void *b,
                                      const void *streams, size_t frame_stride, size_t stream_stride, size_t P, size_t max_stream)
{
    if (!r || !g || !b || !streams) return "null pointer";
    if (!ctx_rgb) return "the context is not an RGB one";
    if (cp == 3) return "-cp 3 codes its planes one by one";
    if (n < 1 || n > kRgbMaxFrames) return "n outside 1..21";
    if (stream_stride < max_stream) return "stream stride smaller than a worst-case codestream";
    if (!same_geometry) return "the components' tables differ in geometry: code the planes one by one";
    if (n > 1) {
        if (frame_stride < P) return "frame_stride smaller than a padded plane";
        // plane x of frame f against plane y of frame f + d: the starts (y - x) + d * frame_stride apart, P bytes each
        const uintptr_t pl[3] = { (uintptr_t)r, (uintptr_t)g, (uintptr_t)b };
        for (int d = 1; d < n; d++)
            for (int x = 0; x < 3; x++)
                for (int y = 0; y < 3; y++) {
                    const long long gap = (long long)(pl[y] - pl[x]) + (long long)d * (long long)frame_stride;
                    if (gap > -(long long)P && gap < (long long)P) return "frame_stride makes a frame's planes overlap the next frame's";
                }
    }
    return nullptr;
}
// ... and picsong_encode_rgb_images / picsong_decode_rgb_images, ahead of the check above: everything layout_refusal
// refuses (the padded side is the context's own buffer, 3 P bytes a frame), a grey layout, n beyond 21
inline const char *rgb_images_refusal(int layout, const void *data, size_t pitch, size_t plane_stride, size_t frame_stride, int n, int W,
                                      int H, int AW, int AH)
{
    if (n < 1 || n > kRgbMaxFrames) return "n outside 1..21";
    const size_t P = (size_t)AW * (size_t)AH;
    if (const char *why = layout_refusal(layout, data, pitch, plane_stride, frame_stride, data, 3 * P, n, W, H, AW, AH)) return why;
    if (layout == kLayoutGrey8) return "a grey layout on an RGB call";
    return nullptr;
}
// The launch: grid.x = the row batches of a plane (layout_rows), grid.y = the planes of a planar layout, grid.z = frame;
// the vector form where the image side is 4-byte and the padded side 16-byte aligned, else the per-byte one.
struct LayoutLaunch { LayoutKernel kernel; dim3 grid; bool vec; };
inline LayoutArgs layout_args(int layout, const void *data, size_t pitch, size_t plane_stride, size_t frame_stride, const void *padded,
                              size_t padded_stride, int n, int W, int H, int AW, int AH, int px_max = 0)
{
    LayoutArgs a;
    memset(&a, 0, sizeof a);
    a.img = (uint8_t *)data; a.pitch = pitch;
    a.plane_stride = layout == kLayoutPlanar3 || layout == kLayoutPlanar3_16 ? plane_stride : 0; a.frame_stride = n > 1 ? frame_stride : 0;
    a.px_max = layout_is_rgb16(layout) ? px_max : 0;
    a.pad = (uint8_t *)padded; a.pad_stride = n > 1 ? padded_stride : 0; a.P = (unsigned long long)AW * (unsigned long long)AH;
    a.W = W; a.H = H; a.AW = AW; a.AH = AH;
    a.a16 = ((((uintptr_t)a.img) | a.pitch | a.plane_stride | a.frame_stride) & 15u) == 0 ? 1 : 0;
    return a;
}
// GREY16 (ingest16_kernel / emit16_kernel): a thread a group of 8 samples, 256 groups a workgroup over the padded
// (ingest) or the visible (emit) rows; the vector form where the padded side is 16-byte and the image side 4-byte aligned
inline LayoutLaunch select_layout16(bool ingest, const LayoutArgs &a)
{
    const bool vec = ((((uintptr_t)a.img) | a.pitch | a.frame_stride) & 3u) == 0 && ((((uintptr_t)a.pad) | a.pad_stride) & 15u) == 0;
    const size_t groups = ingest ? (size_t)(a.AW / 8) * (size_t)a.AH : (size_t)((a.W + 7) / 8) * (size_t)a.H;
    const dim3 grid((unsigned)((groups + 255) / 256), 1u, 1u);
    if (ingest) return { vec ? ingest16_kernel<true> : ingest16_kernel<false>, grid, vec };
    return { vec ? emit16_kernel<true> : emit16_kernel<false>, grid, vec };
}
// the 16-bit colour layouts (ingest_rgb16_kernel / emit_rgb16_kernel): the same groups and grid.x, a thread 8 pixels; grid.y
// = the planes of PLANAR3_16; the vector form where the padded side is 16-byte and the image side 4-byte aligned
inline LayoutLaunch select_layout_rgb16(bool ingest, int layout, const LayoutArgs &a)
{
    const bool vec = ((((uintptr_t)a.img) | a.pitch | a.plane_stride | a.frame_stride) & 3u) == 0 && ((((uintptr_t)a.pad) | a.pad_stride) & 15u) == 0;
    const size_t groups = ingest ? (size_t)(a.AW / 8) * (size_t)a.AH : (size_t)((a.W + 7) / 8) * (size_t)a.H;
    const dim3 grid((unsigned)((groups + 255) / 256), layout == kLayoutPlanar3_16 ? 3u : 1u, 1u);
    LayoutKernel k = nullptr;
    switch (layout) {
    case kLayoutPlanar3_16:
        k = ingest ? (vec ? ingest_rgb16_kernel<kLayoutPlanar3_16, true> : ingest_rgb16_kernel<kLayoutPlanar3_16, false>)
                   : (vec ? emit_rgb16_kernel<kLayoutPlanar3_16, true> : emit_rgb16_kernel<kLayoutPlanar3_16, false>);
        break;
    case kLayoutRgb48:
        k = ingest ? (vec ? ingest_rgb16_kernel<kLayoutRgb48, true> : ingest_rgb16_kernel<kLayoutRgb48, false>)
                   : (vec ? emit_rgb16_kernel<kLayoutRgb48, true> : emit_rgb16_kernel<kLayoutRgb48, false>);
        break;
    default:
        k = ingest ? (vec ? ingest_rgb16_kernel<kLayoutRgba64, true> : ingest_rgb16_kernel<kLayoutRgba64, false>)
                   : (vec ? emit_rgb16_kernel<kLayoutRgba64, true> : emit_rgb16_kernel<kLayoutRgba64, false>);
        break;
    }
    return { k, grid, vec };
}
template <template <int, bool> class K>
inline LayoutLaunch select_layout(int layout, const LayoutArgs &a)
{
    const bool vec = ((((uintptr_t)a.img) | a.pitch | a.plane_stride | a.frame_stride) & 3u) == 0 &&
                     ((((uintptr_t)a.pad) | a.pad_stride) & 15u) == 0;
    const unsigned ppt = layout < kLayoutRgb24 ? 16u : 4u, max_rows = layout < kLayoutRgb24 ? 64u : 21u;
    const unsigned rows = layout_rows(((unsigned)a.W + ppt - 1u) / ppt, max_rows);
    const dim3 grid(((unsigned)a.H + rows - 1u) / rows, layout == kLayoutPlanar3 ? 3u : 1u, 1u);
    LayoutKernel k = nullptr;
    switch (layout) {
    case kLayoutGrey8:   k = vec ? K<kLayoutGrey8, true>::fn() : K<kLayoutGrey8, false>::fn(); break;
    case kLayoutPlanar3: k = vec ? K<kLayoutPlanar3, true>::fn() : K<kLayoutPlanar3, false>::fn(); break;
    case kLayoutRgb24:   k = vec ? K<kLayoutRgb24, true>::fn() : K<kLayoutRgb24, false>::fn(); break;
    case kLayoutBgr24:   k = vec ? K<kLayoutBgr24, true>::fn() : K<kLayoutBgr24, false>::fn(); break;
    case kLayoutRgba32:  k = vec ? K<kLayoutRgba32, true>::fn() : K<kLayoutRgba32, false>::fn(); break;
    case kLayoutBgra32:  k = vec ? K<kLayoutBgra32, true>::fn() : K<kLayoutBgra32, false>::fn(); break;
    }
    return { k, grid, vec };
}
template <int L, bool VEC> struct IngestOf { static LayoutKernel fn() { return ingest_kernel<L, VEC>; } };
template <int L, bool VEC> struct EmitOf { static LayoutKernel fn() { return emit_kernel<L, VEC>; } };
static_assert(LayoutTraits<kLayoutGrey8>::max_rows == 64 && LayoutTraits<kLayoutRgb24>::max_rows == 21, "select_layout's rows are the kernels'");
inline LayoutLaunch select_ingest(int layout, const LayoutArgs &a)
{
    if (layout_is_rgb16(layout)) return select_layout_rgb16(true, layout, a);
    return layout == kLayoutGrey16 ? select_layout16(true, a) : select_layout<IngestOf>(layout, a);
}
inline LayoutLaunch select_emit(int layout, const LayoutArgs &a)
{
    if (layout_is_rgb16(layout)) return select_layout_rgb16(false, layout, a);
    return layout == kLayoutGrey16 ? select_layout16(false, a) : select_layout<EmitOf>(layout, a);
}

// ---- the n-frame RGB proxy calls (picsong_decode_rgb_frames_reduced / _window, picsong_decode_rgb_images_reduced /
// _window): what they refuse, as a message; nullptr: the arguments are fine.  The context's side as rgb_frames_refusal
// takes it, wl and the padded size aw x ah with it.
// A window [x, x + w) x [y, y + h) of the padded image at 1/2^reduce: what picsong_decode_rgb_frame_window refuses
inline const char *proxy_window_refusal(int aw, int ah, int wl, int reduce, int x, int y, int w, int h)
{
    if (!reduce_ok(wl, reduce)) return "reduce outside 0..wl - 1";
    if (w < 1 || h < 1) return "the window is empty";
    if (!window_ok(aw >> reduce, ah >> reduce, x, y, w, h)) return "the window is not inside the padded image at this reduce";
    return nullptr;
}
// picsong_decode_rgb_frames_reduced: frame f's three planes of (aw >> reduce) x (ah >> reduce) bytes frame_stride bytes
// after r / g / b -- rgb_frames_refusal's rules with that span in place of P
inline const char *rgb_frames_reduced_refusal(bool ctx_rgb, int cp, bool same_geometry, int n, const void *r, const void *g, const void *b,
                                              const void *streams, size_t frame_stride, size_t stream_stride, size_t max_stream, int aw,
                                              int ah, int wl, int reduce)
{
    if (!r || !g || !b || !streams) return "null pointer";
    if (!reduce_ok(wl, reduce)) return "reduce outside 0..wl - 1";
    const size_t span = (size_t)(aw >> reduce) * (size_t)(ah >> reduce);
    return rgb_frames_refusal(ctx_rgb, cp, same_geometry, n, r, g, b, streams, frame_stride, stream_stride, span, max_stream);
}
// picsong_decode_rgb_frames_window: row i of frame f's windows at r / g / b + f * frame_stride + i * pitch, w bytes; a
// plane spans (h - 1) * pitch + w bytes
inline const char *rgb_frames_window_refusal(bool ctx_rgb, int cp, bool same_geometry, int n, const void *r, const void *g, const void *b,
                                             const void *streams, size_t pitch, size_t frame_stride, size_t stream_stride, size_t max_stream,
                                             int aw, int ah, int wl, int reduce, int x, int y, int w, int h)
{
    if (!r || !g || !b || !streams) return "null pointer";
    if (const char *why = proxy_window_refusal(aw, ah, wl, reduce, x, y, w, h)) return why;
    if (pitch < (size_t)w) return "out_pitch smaller than the window's width";
    const size_t span = (size_t)(h - 1) * pitch + (size_t)w;
    return rgb_frames_refusal(ctx_rgb, cp, same_geometry, n, r, g, b, streams, frame_stride, stream_stride, span, max_stream);
}
// picsong_decode_rgb_images_window (and _reduced, its window (0, 0, rw, rh)): the w x h window in a colour layout of
// picsong_image -- layout_refusal's rules on a w x h image, no grey layout.  deep_rgb (a deep RGB context): PLANAR3_16,
// RGB48 and RGBA64 and nothing else; they are unknown layouts to every other context
inline const char *rgb_images_window_refusal(bool ctx_rgb, int cp, bool same_geometry, int n, const void *streams, size_t stream_stride,
                                             size_t max_stream, int aw, int ah, int wl, int reduce, int x, int y, int w, int h, int layout,
                                             const void *data, size_t pitch, size_t plane_stride, size_t frame_stride, bool deep_rgb = false)
{
    if (!data || !streams) return "null pointer";
    if (!ctx_rgb) return "the context is not an RGB one";
    if (cp == 3) return "-cp 3 codes its planes one by one";
    if (n < 1 || n > kRgbMaxFrames) return "n outside 1..21";
    if (const char *why = proxy_window_refusal(aw, ah, wl, reduce, x, y, w, h)) return why;
    if (stream_stride < max_stream) return "stream stride smaller than a worst-case codestream";
    if (!same_geometry) return "the components' tables differ in geometry: code the planes one by one";
    if (layout == kLayoutGrey8) return "a grey layout on an RGB call";
    return layout_refusal(layout, data, pitch, plane_stride, frame_stride, data, (deep_rgb ? 6 : 3) * (size_t)w * (size_t)h, n, w, h, w, h,
                          deep_rgb, deep_rgb);
}

// picsong_decode_rgb_images_reduced's route: the reduced sequence into aligned planar planes, then emit_frames with the
// geometry (rw, rh, paw, pah), where every group emit_kernel loads lies within a row of paw bytes and is aligned -- paw a
// multiple of 16 (any 4K or 8K frame up to r = 4); else the window (0, 0, rw, rh).  The bytes are the same.
inline bool reduced_emit_ok(int aw, int reduce) { return ((aw >> reduce) & 15) == 0; }

// Their epilogue (window_rgb_image_kernel, window_kernels.hpp): 256 threads, a thread four adjacent pixels of a row,
// grid.x over the rows' groups, grid.z = frame.  d0 .. d2: frame 0's R, G, B planes (kLayoutPlanar3) or d0 its pixels.
// The vector form where every store address is 4-byte aligned: pointers, pitch and, n > 1, the frame stride.
using WinRgbKernel = void (*)(WinRgbArgs);
struct WinRgbLaunch { WinRgbKernel kernel; dim3 grid; bool vec; };
inline WinRgbArgs window_rgb_args(int layout, const void *work, unsigned long long z_stride, int w, int h, uint8_t *d0, uint8_t *d1,
                                  uint8_t *d2, size_t pitch, size_t frame_stride, unsigned n, int off)
{
    WinRgbArgs a;
    memset(&a, 0, sizeof a);
    a.work = work; a.z_stride = z_stride; a.w = w; a.h = h;
    a.src16 = (w & 3) == 0 && ((((uintptr_t)work) | z_stride) & 15u) == 0 ? 1 : 0;
    a.dst[0] = d0;
    a.dst[1] = layout == kLayoutPlanar3 ? d1 : d0;
    a.dst[2] = layout == kLayoutPlanar3 ? d2 : d0;
    a.pitch = pitch; a.frame_stride = n > 1 ? frame_stride : 0; a.off = off;
    a.a16 = ((((uintptr_t)a.dst[0]) | ((uintptr_t)a.dst[1]) | ((uintptr_t)a.dst[2]) | a.pitch | a.frame_stride) & 15u) == 0 ? 1 : 0;
    return a;
}
template <int L>
inline WinRgbKernel window_rgb_kernel_of(bool lossy, bool vec)
{
    if (lossy) return vec ? window_rgb_image_kernel<float, L, true> : window_rgb_image_kernel<float, L, false>;
    return vec ? window_rgb_image_kernel<int, L, true> : window_rgb_image_kernel<int, L, false>;
}
inline WinRgbLaunch select_window_rgb(bool lossy, int layout, const WinRgbArgs &a, unsigned n)
{
    const bool vec = ((((uintptr_t)a.dst[0]) | ((uintptr_t)a.dst[1]) | ((uintptr_t)a.dst[2]) | a.pitch | a.frame_stride) & 3u) == 0;
    const size_t groups = (size_t)((a.w + 3) / 4) * (size_t)a.h;
    const dim3 grid((unsigned)((groups + 255) / 256), 1u, n);
    WinRgbKernel k = nullptr;
    switch (layout) {
    case kLayoutPlanar3: k = window_rgb_kernel_of<kLayoutPlanar3>(lossy, vec); break;
    case kLayoutRgb24:   k = window_rgb_kernel_of<kLayoutRgb24>(lossy, vec); break;
    case kLayoutBgr24:   k = window_rgb_kernel_of<kLayoutBgr24>(lossy, vec); break;
    case kLayoutRgba32:  k = window_rgb_kernel_of<kLayoutRgba32>(lossy, vec); break;
    case kLayoutBgra32:  k = window_rgb_kernel_of<kLayoutBgra32>(lossy, vec); break;
    }
    return { k, grid, vec };
}

// ---- the deep proxy calls (picsong_decode_frames16_reduced / _window, picsong_decode_rgb_frames16_reduced / _window):
// uint16 samples, every pitch and stride in BYTES.  What they refuse, as a message that names the call to use instead
// where the context is of another kind; nullptr: the arguments are fine.
// The context's side: bit_depth 9..16, grey for the grey pair and RGB for the RGB pair, -cp 2
inline const char *deep_proxy_ctx_refusal(int bit_depth, bool ctx_rgb, bool want_rgb, int cp, bool window)
{
    if (!deep_depth_ok(bit_depth)) {
        if (want_rgb) return window ? "uint16 samples want a deep RGB context (bit_depth 9..16): an 8-bit context's call is picsong_decode_rgb_frames_window"
                                    : "uint16 samples want a deep RGB context (bit_depth 9..16): an 8-bit context's call is picsong_decode_rgb_frames_reduced";
        return window ? "uint16 samples want a deep context (bit_depth 9..16): an 8-bit context's call is picsong_decode_frames_window"
                      : "uint16 samples want a deep context (bit_depth 9..16): an 8-bit context's call is picsong_decode_frames_reduced";
    }
    if (ctx_rgb && !want_rgb)
        return window ? "grey frames on an RGB context: its call is picsong_decode_rgb_frames16_window"
                      : "grey frames on an RGB context: its call is picsong_decode_rgb_frames16_reduced";
    if (!ctx_rgb && want_rgb)
        return window ? "the context is not an RGB one: its call is picsong_decode_frames16_window"
                      : "the context is not an RGB one: its call is picsong_decode_frames16_reduced";
    if (cp == 3) return "-cp 3 contexts decode whole planes only (picsong_decode_plane)";
    return nullptr;
}
// n grey frames of `span` bytes each (the reduced plane, or the window's (h - 1) * pitch + 2 w), frame_stride bytes apart
inline const char *frames16_span_refusal(int n, const void *out, const void *streams, size_t frame_stride, size_t stream_stride,
                                         size_t max_stream, size_t span)
{
    if (n < 1 || n > 64) return "n outside 1..64";
    if ((((uintptr_t)out) | ((uintptr_t)streams)) & 1u) return "pointers need 2-byte alignment";
    if (n > 1 && (frame_stride & 1u)) return "frame_stride must be even";
    if (n > 1 && frame_stride < span) return "frame_stride smaller than a frame's samples";
    if (n > 1 && stream_stride < max_stream) return "stream stride smaller than a worst-case codestream";
    return nullptr;
}
inline const char *frames16_reduced_refusal(int bit_depth, bool ctx_rgb, int cp, int n, const void *out, const void *streams, size_t frame_stride,
                                            size_t stream_stride, size_t max_stream, int aw, int ah, int wl, int reduce)
{
    if (const char *why = deep_proxy_ctx_refusal(bit_depth, ctx_rgb, false, cp, false)) return why;
    if (!out || !streams) return "null pointer";
    if (!reduce_ok(wl, reduce)) return "reduce outside 0..wl - 1";
    return frames16_span_refusal(n, out, streams, frame_stride, stream_stride, max_stream, 2 * (size_t)(aw >> reduce) * (size_t)(ah >> reduce));
}
inline const char *frames16_window_refusal(int bit_depth, bool ctx_rgb, int cp, int n, const void *out, const void *streams, size_t pitch,
                                           size_t frame_stride, size_t stream_stride, size_t max_stream, int aw, int ah, int wl, int reduce,
                                           int x, int y, int w, int h)
{
    if (const char *why = deep_proxy_ctx_refusal(bit_depth, ctx_rgb, false, cp, true)) return why;
    if (!out || !streams) return "null pointer";
    if (const char *why = proxy_window_refusal(aw, ah, wl, reduce, x, y, w, h)) return why;
    if (pitch & 1u) return "out_pitch must be even";
    if (pitch < 2 * (size_t)w) return "out_pitch smaller than the window's row of 2 w bytes";
    return frames16_span_refusal(n, out, streams, frame_stride, stream_stride, max_stream, (size_t)(h - 1) * pitch + 2 * (size_t)w);
}
// the RGB pair: rgb_frames_refusal's rules on planes of `span` bytes, and the alignment of 2-byte samples
inline const char *rgb_frames16_span_refusal(int cp, bool same_geometry, int n, const void *r, const void *g, const void *b, const void *streams,
                                             size_t frame_stride, size_t stream_stride, size_t max_stream, size_t span)
{
    if (const char *why = rgb_frames_refusal(true, cp, same_geometry, n, r, g, b, streams, frame_stride, stream_stride, span, max_stream)) return why;
    if ((((uintptr_t)r) | ((uintptr_t)g) | ((uintptr_t)b) | ((uintptr_t)streams)) & 1u) return "pointers need 2-byte alignment";
    if (n > 1 && (frame_stride & 1u)) return "frame_stride must be even";
    return nullptr;
}
inline const char *rgb_frames16_reduced_refusal(int bit_depth, bool ctx_rgb, int cp, bool same_geometry, int n, const void *r, const void *g,
                                                const void *b, const void *streams, size_t frame_stride, size_t stream_stride,
                                                size_t max_stream, int aw, int ah, int wl, int reduce)
{
    if (const char *why = deep_proxy_ctx_refusal(bit_depth, ctx_rgb, true, cp, false)) return why;
    if (!r || !g || !b || !streams) return "null pointer";
    if (!reduce_ok(wl, reduce)) return "reduce outside 0..wl - 1";
    return rgb_frames16_span_refusal(cp, same_geometry, n, r, g, b, streams, frame_stride, stream_stride, max_stream,
                                     2 * (size_t)(aw >> reduce) * (size_t)(ah >> reduce));
}
inline const char *rgb_frames16_window_refusal(int bit_depth, bool ctx_rgb, int cp, bool same_geometry, int n, const void *r, const void *g,
                                               const void *b, const void *streams, size_t pitch, size_t frame_stride, size_t stream_stride,
                                               size_t max_stream, int aw, int ah, int wl, int reduce, int x, int y, int w, int h)
{
    if (const char *why = deep_proxy_ctx_refusal(bit_depth, ctx_rgb, true, cp, true)) return why;
    if (!r || !g || !b || !streams) return "null pointer";
    if (const char *why = proxy_window_refusal(aw, ah, wl, reduce, x, y, w, h)) return why;
    if (pitch & 1u) return "out_pitch must be even";
    if (pitch < 2 * (size_t)w) return "out_pitch smaller than the window's row of 2 w bytes";
    return rgb_frames16_span_refusal(cp, same_geometry, n, r, g, b, streams, frame_stride, stream_stride, max_stream,
                                     (size_t)(h - 1) * pitch + 2 * (size_t)w);
}

// Their colour epilogue (window_rgb16_image_kernel, window_kernels.hpp): select_window_rgb's grid -- 256 threads, a thread
// four adjacent pixels of a row, grid.x over the rows' groups, grid.z = frame.  d0 .. d2: frame 0's R, G, B planes
// (kLayoutPlanar3_16) or d0 its pixels (kLayoutRgb48, kLayoutRgba64).  The vector form where every store address is 4-byte
// aligned: pointers, pitch and, n > 1, the frame stride; a8: 8-byte aligned as well (dwordx2 stores).
using WinRgb16Kernel = void (*)(WinRgb16Args);
struct WinRgb16Launch { WinRgb16Kernel kernel; dim3 grid; bool vec; };
inline WinRgb16Args window_rgb16_args(int layout, const void *work, unsigned long long z_stride, int w, int h, uint8_t *d0, uint8_t *d1,
                                      uint8_t *d2, size_t pitch, size_t frame_stride, unsigned n, int off, int px_max)
{
    WinRgb16Args a;
    memset(&a, 0, sizeof a);
    a.work = work; a.z_stride = z_stride; a.w = w; a.h = h;
    a.src16 = (w & 3) == 0 && ((((uintptr_t)work) | z_stride) & 15u) == 0 ? 1 : 0;
    a.dst[0] = d0;
    a.dst[1] = layout == kLayoutPlanar3_16 ? d1 : d0;
    a.dst[2] = layout == kLayoutPlanar3_16 ? d2 : d0;
    a.pitch = pitch; a.frame_stride = n > 1 ? frame_stride : 0; a.off = off; a.mx = px_max;
    a.a8 = ((((uintptr_t)a.dst[0]) | ((uintptr_t)a.dst[1]) | ((uintptr_t)a.dst[2]) | a.pitch | a.frame_stride) & 7u) == 0 ? 1 : 0;
    return a;
}
template <int L>
inline WinRgb16Kernel window_rgb16_kernel_of(bool lossy, bool vec)
{
    if (lossy) return vec ? window_rgb16_image_kernel<float, L, true> : window_rgb16_image_kernel<float, L, false>;
    return vec ? window_rgb16_image_kernel<int, L, true> : window_rgb16_image_kernel<int, L, false>;
}
inline WinRgb16Launch select_window_rgb16(bool lossy, int layout, const WinRgb16Args &a, unsigned n)
{
    const bool vec = ((((uintptr_t)a.dst[0]) | ((uintptr_t)a.dst[1]) | ((uintptr_t)a.dst[2]) | a.pitch | a.frame_stride) & 3u) == 0;
    const size_t groups = (size_t)((a.w + 3) / 4) * (size_t)a.h;
    const dim3 grid((unsigned)((groups + 255) / 256), 1u, n);
    WinRgb16Kernel k = nullptr;
    switch (layout) {
    case kLayoutPlanar3_16: k = window_rgb16_kernel_of<kLayoutPlanar3_16>(lossy, vec); break;
    case kLayoutRgb48:      k = window_rgb16_kernel_of<kLayoutRgb48>(lossy, vec); break;
    case kLayoutRgba64:     k = window_rgb16_kernel_of<kLayoutRgba64>(lossy, vec); break;
    }
    return { k, grid, vec };
}

// workgroups (256 threads) of the element-wise kernels -- level shift, clamp, RGB transforms -- over n items, grid-stride
// beyond `cap`
inline unsigned elementwise_blocks(size_t n, unsigned cap = 8192)
{
    const size_t b = (n + 255) / 256;
    return (unsigned)(b > cap ? cap : b);
}

}  // namespace picsong
