// TEST INFRASTRUCTURE ONLY -- the reduced-resolution decode (picsong_decode_frame_reduced, picsong_decode_frames_reduced)
// on the CPU wave emulator: the library's own sequence (decode_frames, launch_seq.hpp) over a context of this file's
// making (emu_decode_ctx.hpp), with the plan functions (launch_plan.hpp), choice of kernel, grid and scratch
// (kernel_select.hpp) and kernel sources of cuda-image-and-video-codec_amd/csrc/picsong_hip.hip, run through the emulator's
// launcher.
// Built by tests/test_reduced_decode_emulated.py with the flags of tests/hipemu/Makefile.
#include "emu_decode_ctx.hpp"

extern "C" {

void emu_reduced_dims(int w, int h, int aw, int ah, int r, int *d) { reduced_dims(w, h, aw, ah, r, d); }
int emu_reduce_ok(int wl, int r) { return reduce_ok(wl, r) ? 1 : 0; }
int emu_reduce_launches(void) { return g_launches; }
void emu_reduce_reset(void) { g_launches = 0; }

// n frames at 1/2^r resolution, as picsong_decode_frames_reduced runs them (n = 1: picsong_decode_frame_reduced): the
// lengths and offsets of the whole streams, stream_shorts apart, the decoder over the rectangle's codeblocks (k = 0 or
// -k > 0; from the streams themselves, or through the staging when `staging` is set), the synthesis levels wl - 1 .. r,
// pixels out of level r.
// geo: the LUT geometry as emu_driver.cpp takes it.  want_c16: the context would take the 16-bit form (c16_dec).
// coef: the decoder's output arrays (n x AW * AH int32), filled by the caller -- what they hold outside the rectangle
// shows what was written.  pixels: frame f's (AW >> r) * (AH >> r) bytes at + f * frame_stride.
// Returns bit 0: level r wrote the pixels (fused store), bit 1: the 16-bit coefficient form, bit 2: levels r + 1 and r
// ran as one launch (dwt_inv2_kernel), bit 3: the lengths were damaged.
int emu_decode_reduced(const uint16_t *stream, unsigned stream_shorts, int aw, int ah, int wl, int lossy, float qs,
                       const int32_t *lut, const int *geo, float k, int n_tables, int want_c16, int staging, int r,
                       int32_t *coef, uint8_t *pixels, int *flag, int n, size_t frame_stride)
{
    Ctx c(n, false, aw, ah, wl, lossy, qs, lut, nullptr, nullptr, geo, k, n_tables, flag, stream_shorts, staging != 0, coef);
    DecodeReport rep;
    if (decode_frames(go, c.g, c.a, c.w, (unsigned)n, stream, stream_shorts, r, nullptr, want_c16 && c.c16(r), true, pixels, frame_stride, 0,
                      &rep)) return -1;
    return (rep.pixels ? 1 : 0) | (rep.c16 ? 2 : 0) | (rep.fused10 ? 4 : 0) | (c.bad ? 8 : 0);
}

}  // extern "C"
