// TEST INFRASTRUCTURE ONLY -- the k = 0 encoder's plane records (bpc_kernels.hpp: plane_record, plane_img_kernel,
// plane_lut_img) and the one-wave-a-codeblock pack on the CPU wave emulator, launched by the sequences picsong_hip.hip
// launches them by (launch_seq.hpp: launch_encoder, widen_staging, pack_frames) through the emulator's launcher.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../cuda-image-and-video-codec_amd/csrc/launch_seq.hpp"

using namespace picsong;

static const emu::Go go{};

extern "C" int emu_plane_img_recs(int wl) { return plane_img_recs(wl); }

// the records as picsong_ctx_set_lut_component builds them (host) or as plane_img_kernel does (a caller's device table)
extern "C" void emu_plane_img_build(const int32_t *lut, const int *geo, int wl, int by_kernel, uint32_t *out)
{
    const LutGeo g = lut_geo(geo);
    PlaneRec *img = reinterpret_cast<PlaneRec *>(out);
    if (by_kernel) go(plane_img_kernel, dim3(1), 256u, lut, g, wl, img);
    else for (int i = 0; i < plane_img_recs(wl); i++) img[i] = plane_record(lut, g, i / kMaxPlanes, i % kMaxPlanes);
}

// plane_lut<true> over the byte copy of the table the coders keep in LDS: {sig0, sig1, sig8, sign, ref, sig8x4}
extern "C" void emu_plane_lut_ref(const int32_t *lut, const int *geo, int grp, int bp, uint32_t *out)
{
    const LutGeo g = lut_geo(geo);
    const int total = g.nRef + g.nSig + g.nSign;
    std::vector<uint8_t> bytes((size_t)total);
    for (int i = 0; i < total; i++) bytes[i] = (uint8_t)((uint32_t)lut[i] & 0xFFu);
    const LutView lv = { bytes.data(), lut, total, total, 0 };
    const PlaneLut pl = plane_lut<true>(lv, g, grp, bp);
    out[0] = pl.sig0; out[1] = pl.sig1; out[2] = pl.sig8; out[3] = pl.sign; out[4] = pl.ref; out[5] = pl.sig8x4;
}

// what the encoder reads from the image for (slot, bp), same order
extern "C" void emu_plane_lut_img(const uint32_t *img, int slot, int bp, uint32_t *out)
{
    const PlaneLut pl = plane_lut_img(reinterpret_cast<const PlaneRec *>(img), slot, bp);
    out[0] = pl.sig0; out[1] = pl.sig1; out[2] = pl.sig8; out[3] = pl.sign; out[4] = pl.ref; out[5] = pl.sig8x4;
}

// k = 0 encode of `frames` frames in ONE launch, frame f with table luts[f] and its image (the batched launch of
// picsong_encode_rgb_frame: whole workgroups a frame; frames = 1: bpc_encode_impl's launch).  coeffs: int32 Mallat
// arrays one after the other; staging / sizes: per frame, int32[aw * ah] / int32[nCB], as picsong_bpc_encode leaves them.
extern "C" void emu_bpc_encode_img(const int32_t *coeffs, int aw, int ah, int wl, const int32_t *const *luts, const int *geo,
                                   int frames, int32_t *staging, int32_t *sizes, int *flag)
{
    const LutGeo g = lut_geo(geo);
    const int ncb = (aw / 64) * (ah / 64), wpf = (ncb + 1) / 2;
    std::vector<std::vector<PlaneRec>> imgs((size_t)frames);
    for (int f = 0; f < frames; f++) {
        imgs[f].resize((size_t)plane_img_recs(wl));
        for (int i = 0; i < plane_img_recs(wl); i++) imgs[f][i] = plane_record(luts[f], g, i / kMaxPlanes, i % kMaxPlanes);
    }
    BpcArgs a = bpc_frame_args(aw, ah, wl, luts[0], g, flag);
    a.sizes = sizes; a.coeffs_in = coeffs;
    a.k = 0.0f; a.n_tables = 1;
    a.plane_img = imgs[0].data();
    std::vector<uint16_t> st16((size_t)frames * (size_t)aw * (size_t)ah, 0xDEADu);     // poisoned
    a.staging16 = st16.data();
    unsigned waves = (unsigned)wpf;
    if (frames > 1) {
        a.frames = frames; a.waves_per_frame = (wpf + kBpcEncWgWaves - 1) / kBpcEncWgWaves * kBpcEncWgWaves;
        a.coef_z = (unsigned long long)aw * (unsigned long long)ah * 4ull;
        for (int f = 0; f < frames && f < 3; f++) { a.lut_c[f] = luts[f]; a.img_c[f] = imgs[f].data(); }
        waves = (unsigned)(frames * a.waves_per_frame);
    }
    std::vector<uint32_t> plane_scratch(encoder_scratch_dwords(false, false, waves), 0xDEADBEEFu);
    a.plane_scratch = plane_scratch.data();
    launch_encoder(go, a, false, false, waves);
    memset(staging, 0xFF, (size_t)frames * (size_t)aw * (size_t)ah * 4);
    for (int f = 0; f < frames; f++)
        widen_staging(go, st16.data() + (size_t)f * aw * ah, sizes + (size_t)f * ncb, 0, ncb, staging + (size_t)f * aw * ah);
}

// scan + pack of `frames` frames from 16-bit staging with the library's grid: pack_blocks<uint16_t>(ncb) workgroups of
// four waves a frame.  out: frames x out_stride shorts; header on frame 0 when given.  Returns frame 0's total.
extern "C" int emu_pack16_frames(const uint16_t *staging16, const int32_t *sizes, int ncb, int frames, const uint16_t *header,
                                 uint16_t *out, size_t out_stride, int32_t *totals)
{
    std::vector<int32_t> offsets((size_t)ncb * frames);
    const Workspace w = { nullptr, nullptr, const_cast<int32_t *>(sizes), offsets.data(), totals, nullptr, nullptr };
    pack_frames(go, staging16, w, ncb, (unsigned)frames, header, 1, out, (size_t)ncb * 4096u, out_stride);
    return totals[0];
}
