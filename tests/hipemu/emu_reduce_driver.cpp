// TEST INFRASTRUCTURE ONLY -- the reduced-resolution decode (picsong_decode_frame_reduced) on the CPU wave emulator:
// the decoder over the codeblock rectangle of the 1/2^r image's corner and the synthesis stopped at level r, through
// the same plan functions (launch_plan.hpp), the same choice of kernel, grid and scratch (kernel_select.hpp) and the same
// kernel sources as cuda-image-and-video-codec_amd/csrc/picsong_hip.hip.
// Built by tests/test_reduced_decode_emulated.py with the flags of tests/hipemu/Makefile.
#include <hip/hip_runtime.h>

#include "../../cuda-image-and-video-codec_amd/csrc/kernel_select.hpp"

using namespace picsong;

extern "C" {

void emu_reduced_dims(int w, int h, int aw, int ah, int r, int *d) { reduced_dims(w, h, aw, ah, r, d); }
int emu_reduce_ok(int wl, int r) { return reduce_ok(wl, r) ? 1 : 0; }

// One frame at 1/2^r resolution, as picsong_decode_frame_reduced runs it: the lengths and offsets of the whole stream
// (scan_stream_kernel), the decoder over the rectangle's codeblocks (k = 0 or -k > 0; from the stream itself, or
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
    const size_t extra = [&] { size_t e = 0; for (int l = 1; l < wl; l++) e += (size_t)(aw >> l) * (size_t)(ah >> l); return e; }();
    std::vector<float> scratch((size_t)aw * ah + extra + 16, std::nanf(""));
    void *wrk = (void *)(((uintptr_t)scratch.data() + 63) & ~(uintptr_t)63);

    // ---- synthesis plan first (inverse_plan): it decides whether the coefficients travel as int16
    const bool px = (((uintptr_t)pixels) & 3u) == 0;
    std::vector<InvLaunch> plan = plan_dwt_inverse_reduced(coef, wrk, aw, ah, wl, qs, fast, c16 && px, r);
    int res = 0;
    if (px && plan.back().vec) { plan.back().a.dst_u8 = pixels; plan.back().a.off = 128; res |= 1; }
    const bool c16p = plan_inv_is_c16(plan);
    if (c16p) res |= 2;

    // ---- decoder over the rectangle
    std::vector<int32_t> sizes(ncb), offsets(ncb), stage;
    int32_t total = 0;
    int bad = 0;
    BpcArgs a = bpc_frame_args(aw, ah, wl, lut, lut_geo(geo), flag);
    a.sizes = sizes.data(); a.coeffs_out = coef;
    a.k = k; a.n_tables = n_tables;
    if (r > 0) {
        const ReducedRect q = reduced_rect(aw, ah, r);
        a.ncx_r = q.ncx_r; a.ncb_r = q.ncx_r * q.ncy_r;
    }
    const unsigned waves = (unsigned)(r > 0 ? reduced_waves(reduced_rect(aw, ah, r)) : (ncb + 1) / 2);
    if (staging) {
        stage.assign((size_t)ncb * 4096, 0);
        emu::launch(dim3((unsigned)((ncb + 255) / 256)), dim3(256), [&] { read_sizes_kernel(stream, ncb, sizes.data(), &bad); });
        emu::launch(dim3(1), dim3(scan_threads(ncb)), [&] { scan_sizes_kernel(sizes.data(), ncb, offsets.data(), &total); });
        emu::launch(dim3((unsigned)ncb), dim3(256), [&] { unpack_kernel(stream, sizes.data(), offsets.data(), ncb, stage.data()); });
        a.staging = stage.data();
    } else {
        emu::launch(dim3(1), dim3(scan_threads(ncb)), [&] { scan_stream_kernel(stream, ncb, sizes.data(), offsets.data(), &total, &bad, 0); });
        a.cw16 = stream; a.cw16_offsets = offsets.data(); a.cw16_total = &total; a.cw16_max = stream_shorts;
    }
    if (bad) res |= 8;
    const BpcLaunch dec = select_decoder(false, k > 0.0f, k > 0.0f && bulk_compact(aw, ah, wl, a.g), !staging, c16p, waves);
    std::vector<uint32_t> ps(dec.scratch_dwords, 0xDEADBEEFu);
    a.plane_scratch = ps.data();
    emu::launch(dim3(dec.wgs), dim3(dec.threads), [&] { dec.kernel(a); });

    // ---- synthesis (run_inverse), then the clamp where level r did not write the pixels itself
    Inv2Launch f2;
    const bool fused = plan_dwt_inv2(plan, f2, lossy != 0);
    const size_t n = fused ? plan.size() - 2 : plan.size();
    for (size_t l = 0; l < n; l++) {        // (the frame paths' levels: the lean 9/7 kernel where it applies)
        const InvKernel kl = select_inv(lossy != 0, true, plan[l]);
        emu::launch(dim3(plan[l].gx, plan[l].gy), dim3(256), [&] { kl(plan[l].a); });
    }
    if (fused) {
        const Inv2Kernel k2 = select_inv2(lossy != 0, f2.a.l0.one_div != 0);
        emu::launch(dim3(f2.gx, f2.gy), dim3(256), [&] { k2(f2.a); });
        res |= 4;
    }
    if (!(res & 1)) {
        const size_t n4 = (size_t)(aw >> r) * (size_t)(ah >> r) / 4;
        const void *img = plan.back().a.dst;
        if (lossy) emu::launch(dim3(elementwise_blocks(n4)), dim3(256), [&] { clamp_to_u8_f32_kernel((const float *)img, pixels, n4, 128.0f); });
        else emu::launch(dim3(elementwise_blocks(n4)), dim3(256), [&] { clamp_to_u8_i32_kernel((const int32_t *)img, pixels, n4, 128); });
    }
    return res;
}

}  // extern "C"
