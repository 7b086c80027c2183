// TEST INFRASTRUCTURE ONLY -- what the frame-decode drivers (emu_reduce_driver.cpp, emu_window_driver.cpp,
// emu_rgb_frames_driver.cpp, emu_rgb_proxy_driver.cpp) share: the launcher that counts its launches, and what
// picsong_hip.hip keeps in a context for the decode sequences of launch_seq.hpp -- the buffers (poisoned), the tables on one
// coder grid, the switches.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../cuda-image-and-video-codec_amd/csrc/launch_seq.hpp"

using namespace picsong;

static int g_launches = 0;
struct CountGo {
    template <typename K, typename... A>
    int operator()(K k, dim3 grid, unsigned threads, const A &...args) const
    {
        g_launches++;
        return emu::Go{}(k, grid, threads, args...);
    }
};
static const CountGo go{};

static inline size_t max_stream_shorts(int aw, int ah) { return 9 + 2 * (size_t)(aw / 64) * (size_t)(ah / 64) + (size_t)aw * (size_t)ah + 1; }

// the coder's tables of a context: one (grey: luts[1] == nullptr) or the three components' on one grid (bpc_args_rgb)
static inline BpcArgs table_args(int aw, int ah, int wl, const int32_t *const *luts, const int *geo, float k, int n_tables, int *flag)
{
    BpcArgs a = bpc_frame_args(aw, ah, wl, luts[0], lut_geo(geo), flag);
    a.k = k; a.n_tables = n_tables;
    for (int c = 0; c < 3 && luts[1]; c++) { a.lut_c[c] = luts[c]; a.img_c[c] = nullptr; }
    return a;
}
// bulk_compact of picsong_hip.hip: PICSONG_BULK_FULLTAB=1 keeps the whole-table instantiations
static inline bool emu_compact(int aw, int ah, int wl, const int *geo, float k)
{
    if (const char *e = getenv("PICSONG_BULK_FULLTAB")) if (atoi(e) != 0) return false;
    return k > 0.0f && bulk_compact(aw, ah, wl, lut_geo(geo));
}

// a decode context of n frames (rgb: 3 n planes): its buffers, poisoned, and what decode_ctx (picsong_hip.hip) hands the
// sequences.  coef_out: the caller's array for the decoded coefficients (else the context's own); staging: the decoder
// reads the staging, not the streams; in_max: the samples' range (128 grey, 255 colour) for dec_c16_ok.
struct Ctx {
    std::vector<int32_t> coef_i, work, stage, sizes, offsets, totals;
    std::vector<uint32_t> scratch;
    Workspace w;
    DecodeCtx g;
    BpcArgs a;
    int bad = 0;
    Ctx(int n, bool rgb, int aw, int ah, int wl, int lossy, float qs, const int32_t *lut0, const int32_t *lut1, const int32_t *lut2,
        const int *geo, float k, int n_tables, int *flag, uint32_t max_stream, bool staging = false, int32_t *coef_out = nullptr)
    {
        const size_t P = (size_t)aw * ah, extra = dwt_extra(aw, ah, wl);
        const int ncb = (aw / 64) * (ah / 64);
        const unsigned np = (rgb ? 3u : 1u) * (unsigned)n;
        if (!coef_out) coef_i.assign((size_t)np * P, 0x5A5A5A5A);
        work.assign((size_t)np * (P + extra) + 16, 0x5A5A5A5A);
        if (staging) stage.assign((size_t)np * P, 0);
        sizes.assign((size_t)np * ncb, -7); offsets.assign((size_t)np * ncb, -7); totals.assign(np, -7);
        // (whole workgroups a plane, every codeblock pair or the most a window lists: dec_waves of a context)
        const unsigned wpf = (unsigned)std::max(rgb_component_waves(k > 0.0f, (ncb + 1) / 2), window_waves_cap(aw, ah, wl, lossy != 0, ncb, 4));
        scratch.assign(decoder_scratch_dwords(false, k > 0.0f, np * wpf), 0xDEADBEEFu);
        void *const wrk = (void *)(((uintptr_t)work.data() + 63) & ~(uintptr_t)63);
        w = Workspace{ wrk, staging ? stage.data() : nullptr, sizes.data(), offsets.data(), totals.data(), scratch.data(),
                       coef_out ? coef_out : coef_i.data() };
        const int32_t *luts[3] = { lut0, lut1, lut2 };
        a = table_args(aw, ah, wl, luts, geo, k, n_tables, flag);
        g.aw = aw; g.ah = ah; g.wl = wl; g.ncb = ncb;
        g.lossy = lossy != 0; g.qs = qs; g.fast_div = lossy && dequant_fast_ok(qs, wl); g.off = 128;
        g.P = P; g.extra = extra; g.rgb = rgb; g.cp3 = false; g.direct = !staging; g.compact = emu_compact(aw, ah, wl, geo, k);
        g.max_stream = max_stream; g.flag = &bad;
    }
    // the 16-bit form a context of these parameters would take at 1/2^reduce (c16_dec, dec_c16_reduced)
    bool c16(int reduce) const { return dec_c16_ok(g.lossy, g.wl, g.qs, g.rgb ? 255 : 128, g.aw, g.ah, g.fast_div, reduce); }
};
