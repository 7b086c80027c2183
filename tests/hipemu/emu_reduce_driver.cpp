// TEST INFRASTRUCTURE ONLY -- the reduced-resolution decode (picsong_decode_frame_reduced) on the CPU wave emulator:
// the decoder over the codeblock rectangle of the 1/2^r image's corner and the synthesis stopped at level r, through
// the same launch sequences (launch_seq.hpp: stream_intake, launch_decoder, run_inverse, clamp_pixels), plan functions
// (launch_plan.hpp: plan_inverse_frames), choice of kernel, grid and scratch (kernel_select.hpp) and kernel sources as
// cuda-image-and-video-codec_amd/csrc/picsong_hip.hip, run through the emulator's launcher.
// Built by tests/test_reduced_decode_emulated.py with the flags of tests/hipemu/Makefile.
#include <hip/hip_runtime.h>

#include "../../cuda-image-and-video-codec_amd/csrc/launch_seq.hpp"

using namespace picsong;

static const emu::Go go{};

extern "C" {

void emu_reduced_dims(int w, int h, int aw, int ah, int r, int *d) { reduced_dims(w, h, aw, ah, r, d); }
int emu_reduce_ok(int wl, int r) { return reduce_ok(wl, r) ? 1 : 0; }

// One frame at 1/2^r resolution, as picsong_decode_frame_reduced runs it: the lengths and offsets of the whole stream
// (stream_intake), the decoder over the rectangle's codeblocks (k = 0 or -k > 0; from the stream itself, or
// through the staging when `staging` is set), the synthesis levels wl - 1 .. r, pixels out of level r.
// geo: the LUT geometry as emu_driver.cpp takes it.  want_c16: the context would take the 16-bit form (c16_dec).
// coef: the decoder's output array (AW * AH int32), filled by the caller -- what it holds outside the rectangle shows
// what was written.  pixels: (AW >> r) * (AH >> r) bytes and more; `misalign` bytes into the caller's buffer.
// Returns bit 0: level r wrote the pixels (fused store), bit 1: the 16-bit coefficient form, bit 2: levels r + 1 and r
// ran as one launch (dwt_inv2_kernel), bit 3: the lengths were damaged.
int emu_decode_reduced(const uint16_t *stream, unsigned stream_shorts, int aw, int ah, int wl, int lossy, float qs,
                       const int32_t *lut, const int *geo, float k, int n_tables, int want_c16, int staging, int r,
                       int32_t *coef, uint8_t *pixels, int *flag)
{
    const int ncb = (aw / 64) * (ah / 64);
    const bool fast = lossy && dequant_fast_ok(qs, wl);
    const bool c16 = want_c16 && !staging && dec_c16_ok(lossy != 0, wl, qs, 128, aw, ah, fast, r);
    const size_t P = (size_t)aw * ah, extra = dwt_extra(aw, ah, wl);
    std::vector<float> scratch(P + extra + 16, std::nanf(""));
    void *wrk = (void *)(((uintptr_t)scratch.data() + 63) & ~(uintptr_t)63);

    // ---- synthesis plan first (inverse_plan): it decides whether the coefficients travel as int16
    bool px = false, fused10 = false;
    const std::vector<InvLaunch> plan = plan_inverse_frames(coef, wrk, pixels, &px, 1, 0, c16, false, r, aw, ah, wl, qs, fast, 128, P, extra);
    const bool c16p = plan_inv_is_c16(plan);

    // ---- decoder over the rectangle
    std::vector<int32_t> sizes(ncb), offsets(ncb), stage(staging ? (size_t)ncb * 4096 : 0, 0);
    int32_t total = 0;
    int bad = 0;
    BpcArgs a = bpc_frame_args(aw, ah, wl, lut, lut_geo(geo), flag);
    a.k = k; a.n_tables = n_tables;
    if (r > 0) {
        const ReducedRect q = reduced_rect(aw, ah, r);
        a.ncx_r = q.ncx_r; a.ncb_r = q.ncx_r * q.ncy_r;
    }
    const unsigned waves = (unsigned)(r > 0 ? reduced_waves(reduced_rect(aw, ah, r)) : (ncb + 1) / 2);
    std::vector<uint32_t> ps(decoder_scratch_dwords(false, k > 0.0f, waves), 0xDEADBEEFu);
    const Workspace w = { wrk, stage.data(), sizes.data(), offsets.data(), &total, ps.data(), coef };
    stream_intake(go, stream, 1u, 0, !staging, ncb, P, w, &bad);
    launch_decoder(go, a, false, waves, k > 0.0f && bulk_compact(aw, ah, wl, a.g), w, staging ? nullptr : stream, 0, stream_shorts, c16p);

    // ---- synthesis (the frame paths' levels: the lean 9/7 kernel where it applies), then the clamp where level r did
    // not write the pixels itself
    run_inverse(go, lossy != 0, true, plan, 1, &fused10);
    if (!px) clamp_pixels(go, lossy != 0, plan.back().a.dst, pixels, (size_t)(aw >> r) * (size_t)(ah >> r) / 4, 128);
    return (px ? 1 : 0) | (c16p ? 2 : 0) | (fused10 ? 4 : 0) | (bad ? 8 : 0);
}

}  // extern "C"
