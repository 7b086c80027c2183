// TEST INFRASTRUCTURE ONLY -- runs the product's kernel sources on the CPU wave emulator and
// exposes host-memory entry points (ctypes) so tests can compare them with the oracle without a
// GPU.  Follows the launch sequence of cuda-image-and-video-codec_amd/csrc/picsong_hip.hip; the plans (launch_plan.hpp)
// and the choice of kernel, grid and scratch (kernel_select.hpp) are the library's own.
#include <hip/hip_runtime.h>

#include "../../cuda-image-and-video-codec_amd/csrc/kernel_select.hpp"

using namespace picsong;

// what picsong_ctx_create decides once per context (cached here per (qs, wl))
static bool emu_fast_div(int lossy, float qs, int wl)
{
    static float c_qs = -1.0f;
    static int c_wl = -1;
    static bool c_ok = false;
    if (!lossy) return false;
    if (getenv("PICSONG_DWT_EXACTDIV") || qs != c_qs || wl != c_wl) { c_ok = dequant_fast_ok(qs, wl); c_qs = qs; c_wl = wl; }
    return c_ok;
}
extern "C" int emu_dequant_fast_ok(float qs, int wl) { return dequant_fast_ok(qs, wl) ? 1 : 0; }
// x / c next to the reciprocal form, for the test that sweeps them against each other
extern "C" long emu_div_mismatches(float c, unsigned first_bits, unsigned last_bits, unsigned step)
{
    const volatile float one = 1.0f;
    const float rc = one / c;
    long bad = 0;
    for (uint64_t u = first_bits; u <= last_bits; u += step) {
        float x;
        const uint32_t b = (uint32_t)u;
        memcpy(&x, &b, 4);
        if (div_rc(x, c, rc) != x / c) bad++;
    }
    return bad;
}

// PICSONG_DWT_INV97=0 keeps the 9/7 levels off the lean kernel: read at every call (the tests flip it)
static bool emu_lean97() { const char *e = getenv("PICSONG_DWT_INV97"); return !(e && atoi(e) == 0); }
static void emu_inv(const InvLaunch &f, int lossy)
{
    const InvKernel k = select_inv(lossy != 0, emu_lean97(), f);
    emu::launch(dim3(f.gx, f.gy), dim3(256), [&] { k(f.a); });
}
// levels [from, to) of a synthesis plan
static void emu_inv_levels(const std::vector<InvLaunch> &plan, size_t from, size_t to, int lossy)
{
    for (size_t l = from; l < to; l++) emu_inv(plan[l], lossy);
}
static void emu_inv2(const Inv2Launch &f2, int lossy)
{
    const Inv2Kernel k = select_inv2(lossy != 0, f2.a.l0.one_div != 0);
    emu::launch(dim3(f2.gx, f2.gy), dim3(256), [&] { k(f2.a); });
}

static void emu_fwd(const FwdLaunch &f, int lossy, unsigned frames = 1)
{
    const FwdKernel k = select_fwd(lossy != 0, f);
    emu::launch(dim3(f.gx, f.gy, frames), dim3(256), [&] { k(f.a); });
}

// frame paths: coded coefficients as int16 (DwtFwdArgs::c16 / BpcArgs::c16), switched on by the tests
static int g_c16 = 0;
extern "C" void emu_set_c16(int on) { g_c16 = on; }
extern "C" int emu_coef16_ok(int lossy, int wl, float qs, int in_max, int aw, int ah)
{
    return coef16_ok(lossy != 0, wl, qs, in_max) && dwt_c16_geometry_ok(aw, ah, wl) ? 1 : 0;
}

static void emu_fwd2(const Fwd2Launch &f, int lossy, bool rgb = false)
{
    const Fwd2Kernel k = select_fwd2(lossy != 0, f.a.l0.c16 != 0, rgb);
    emu::launch(dim3(f.gx, f.gy, rgb ? 3u : 1u), dim3(256), [&] { k(f.a); });
}

extern "C" {

// how many levels of the plans take the vector-only kernel instantiations (tests assert on it)
int emu_dwt_vec_levels(const void *in, void *out, int aw, int ah, int wl)
{
    int n = 0;
    for (const FwdLaunch &f : plan_dwt_forward(in, true, out, aw, ah, wl, 1.0f)) n += f.vec ? 1 : 0;
    for (const InvLaunch &f : plan_dwt_inverse((const int32_t *)in, out, aw, ah, wl, 1.0f)) n += f.vec ? 1 : 0;
    return n;
}

static void emu_fwd_levels(const std::vector<FwdLaunch> &plan, size_t from, int lossy, unsigned frames = 1)
{
    for (size_t l = from; l < plan.size(); l++) emu_fwd(plan[l], lossy, frames);
}

// as dwt_forward_impl (picsong_hip.hip); returns 1 when levels 0 and 1 went through the fused kernel
int emu_dwt_forward(const void *in, int u8in, void *out, int aw, int ah, int wl, int lossy, float qs)
{
    const std::vector<FwdLaunch> plan = plan_dwt_forward(in, u8in != 0, out, aw, ah, wl, qs, g_c16 != 0);
    Fwd2Launch f2;
    const bool fused01 = plan_dwt_fwd2(plan, f2, true, lossy != 0);
    if (fused01) emu_fwd2(f2, lossy);
    emu_fwd_levels(plan, fused01 ? 2 : 0, lossy);
    return fused01 ? 1 : 0;
}

// picsong_encode_rgb_frame's transform: the colour transform (RCT / ICT) in the fused head's load stage, one launch for the
// three components (out: three coefficient buffers of `stride` bytes, int16 Mallat arrays at their starts); returns 1
// when the fused form applies
int emu_dwt_forward_rgb(const uint8_t *r, const uint8_t *g, const uint8_t *b, void *out, size_t stride, int aw, int ah, int wl,
                        int lossy, float qs)
{
    std::vector<FwdLaunch> plan = plan_dwt_forward(r, true, out, aw, ah, wl, qs, true);
    for (size_t l = 0; l < plan.size(); l++) {
        plan[l].a.src_z = l == 0 ? 0ull : (unsigned long long)stride;
        plan[l].a.dst_z = (unsigned long long)stride;
    }
    plan[0].a.src_g = g; plan[0].a.src_b = b;
    Fwd2Launch f2;
    if (!plan_is_c16(plan) || !plan_dwt_fwd2(plan, f2, true, lossy != 0, kF2PairsRgb)) return 0;
    emu_fwd2(f2, lossy, true);
    emu_fwd_levels(plan, 2, lossy, 3u);
    return 1;
}

// picsong_dwt_forward_band / picsong_dwt_forward_tail
void emu_dwt_forward_band(const void *in, void *out, int aw, int ah, int wl, int lossy, float qs, int row0, int rows)
{
    std::vector<FwdLaunch> plan = plan_dwt_forward(in, true, out, aw, ah, wl, qs);
    plan_restrict_band(plan[0], row0, rows);
    emu_fwd(plan[0], lossy);
}

void emu_dwt_forward_tail(void *out, int aw, int ah, int wl, int lossy, float qs)
{
    const std::vector<FwdLaunch> plan = plan_dwt_forward(out, false, out, aw, ah, wl, qs);
    emu_fwd_levels(plan, 1, lossy);
}

void emu_dwt_inverse(const int32_t *in, void *out, int aw, int ah, int wl, int lossy, float qs)
{
    for (const InvLaunch &f : plan_dwt_inverse(in, out, aw, ah, wl, qs, emu_fast_div(lossy, qs, wl))) emu_inv(f, lossy);
}

// the frame path's inverse: the finest level writes clamped pixels (inverse_plan + run_inverse, 32-bit coefficients);
// returns 1 when that fused kernel applied
int emu_dwt_inverse_u8(const int32_t *in, void *scratch, uint8_t *pixels, int aw, int ah, int wl, int lossy, float qs)
{
    std::vector<InvLaunch> plan = plan_dwt_inverse(in, scratch, aw, ah, wl, qs, emu_fast_div(lossy, qs, wl));
    const bool fused = !plan.empty() && plan.back().vec && (((uintptr_t)pixels) & 3u) == 0;
    if (fused) { plan.back().a.dst_u8 = pixels; plan.back().a.off = 128; }
    emu_inv_levels(plan, 0, plan.size(), lossy);
    return fused ? 1 : 0;
}

// the decode frame paths with 16-bit coefficients (inverse_plan + run_inverse, picsong_hip.hip): `in16` is an
// int16 Mallat array; returns bit 0: the finest level wrote the pixels, bit 1: levels 1 and 0 ran as ONE launch
// (dwt_inv2_kernel), bit 2: the plan took the 16-bit form (0: the caller's geometry / context does not allow it)
int emu_dwt_inverse_u8_c16(const int16_t *in16, void *scratch, uint8_t *pixels, int aw, int ah, int wl, int lossy, float qs)
{
    const bool fast = emu_fast_div(lossy, qs, wl);
    if (!dec_c16_ok(lossy != 0, wl, qs, 128, aw, ah, fast)) return 0;
    std::vector<InvLaunch> plan = plan_dwt_inverse((const int32_t *)in16, scratch, aw, ah, wl, qs, fast, true);
    if (!plan_inv_is_c16(plan)) return 0;
    int res = 4;
    if (plan.back().vec && (((uintptr_t)pixels) & 3u) == 0) { plan.back().a.dst_u8 = pixels; plan.back().a.off = 128; res |= 1; }
    Inv2Launch f2;
    const bool fused10 = plan_dwt_inv2(plan, f2, lossy != 0);
    emu_inv_levels(plan, 0, fused10 ? plan.size() - 2 : plan.size(), lossy);
    if (fused10) { emu_inv2(f2, lossy); res |= 2; }
    return res;
}

// picsong_decode_rgb_frame's synthesis with 16-bit coefficients (5/3: dwt_inv_rgb_kernel; 9/7: dwt_inv97_rgb_kernel): the levels above the finest per component,
// then the finest level of all three components + the inverse colour transform as ONE launch (dwt_inv_rgb_kernel).
// in16: three int16 Mallat arrays in_z BYTES apart; scratch: three work buffers wrk_z bytes apart.  Returns 1 when the
// form applies.
int emu_dwt_inverse_rgb(const int16_t *in16, size_t in_z, void *scratch, size_t wrk_z, uint8_t *r, uint8_t *g, uint8_t *b,
                        int aw, int ah, int wl, int lossy, float qs)
{
    const bool fast = emu_fast_div(lossy, qs, wl);
    if (!dec_c16_ok(lossy != 0, wl, qs, 255, aw, ah, fast)) return 0;
    std::vector<InvLaunch> plan0;
    for (int c = 0; c < 3; c++) {
        std::vector<InvLaunch> plan = plan_dwt_inverse((const int32_t *)((const char *)in16 + c * in_z), (char *)scratch + c * wrk_z,
                                                       aw, ah, wl, qs, fast, true);
        if (!plan_inv_is_c16(plan) || plan.size() < 2 || !plan.back().vec) return 0;
        emu_inv_levels(plan, 0, plan.size() - 1, lossy);
        if (c == 0) plan0 = plan;
    }
    DwtInvArgs fa = plan0.back().a;
    fa.mallat_z = in_z; fa.ll_z = wrk_z; fa.off = 128;
    // (9/7: the three components as the three waves of a workgroup, dwt_inv97_rgb_kernel)
    const InvRgbLaunch t = select_inv_rgb(lossy != 0, plan0.back());
    emu::launch(dim3(t.gx, t.gy), dim3(t.threads), [&] { t.kernel(fa, r, g, b); });
    return 1;
}

void emu_level_shift_inv(void *data, size_t n, int lossy)
{
    if (lossy) emu::launch(dim3(elementwise_blocks(n)), dim3(256), [&] { level_shift_inv_f32_kernel((float *)data, n, 128.0f); });
    else emu::launch(dim3(elementwise_blocks(n)), dim3(256), [&] { level_shift_inv_i32_kernel((int32_t *)data, n, 128); });
}

void emu_clamp_to_u8(const void *data, uint8_t *out, size_t n, int lossy)
{
    if (lossy) emu::launch(dim3(elementwise_blocks(n / 4)), dim3(256), [&] { clamp_to_u8_f32_kernel((const float *)data, out, n / 4, 128.0f); });
    else emu::launch(dim3(elementwise_blocks(n / 4)), dim3(256), [&] { clamp_to_u8_i32_kernel((const int32_t *)data, out, n / 4, 128); });
}

void emu_rgb_forward(const uint8_t *r, const uint8_t *g, const uint8_t *b, void *c0, void *c1, void *c2, size_t n, int lossy)
{
    if (lossy) emu::launch(dim3(elementwise_blocks(n / 4)), dim3(256), [&] { rgb_forward_kernel<float>(r, g, b, (float *)c0, (float *)c1, (float *)c2, n / 4, 128); });
    else emu::launch(dim3(elementwise_blocks(n / 4)), dim3(256), [&] { rgb_forward_kernel<int32_t>(r, g, b, (int32_t *)c0, (int32_t *)c1, (int32_t *)c2, n / 4, 128); });
}

void emu_rgb_inverse(const void *c0, const void *c1, const void *c2, uint8_t *r, uint8_t *g, uint8_t *b, size_t n, int lossy)
{
    if (lossy) emu::launch(dim3(elementwise_blocks(n / 4)), dim3(256), [&] { rgb_inverse_kernel<float>((const float *)c0, (const float *)c1, (const float *)c2, r, g, b, n / 4, 128); });
    else emu::launch(dim3(elementwise_blocks(n / 4)), dim3(256), [&] { rgb_inverse_kernel<int32_t>((const int32_t *)c0, (const int32_t *)c1, (const int32_t *)c2, r, g, b, n / 4, 128); });
}

void emu_level_shift_fwd(const uint8_t *in, void *out, size_t n, int lossy)
{
    if (lossy) emu::launch(dim3(elementwise_blocks(n / 4, 4096)), dim3(256), [&] { level_shift_fwd_kernel<float>(in, (float *)out, n / 4, 128); });
    else emu::launch(dim3(elementwise_blocks(n / 4, 4096)), dim3(256), [&] { level_shift_fwd_kernel<int32_t>(in, (int32_t *)out, n / 4, 128); });
}

// -k > 0: the COMPACT table copies where the geometry allows them; PICSONG_BULK_FULLTAB=1 keeps the whole tables (read at
// every call, as the library does)
static bool emu_bulk_compact(int aw, int ah, int wl, const int *geo)
{
    if (const char *e = getenv("PICSONG_BULK_FULLTAB")) if (atoi(e) != 0) return false;
    return bulk_compact(aw, ah, wl, lut_geo(geo));
}

static BpcArgs mk(int aw, int ah, int wl, const int32_t *lut, const int *geo, int32_t *staging, int32_t *sizes,
                  int *flag)
{
    BpcArgs a = bpc_frame_args(aw, ah, wl, lut, lut_geo(geo), flag);
    a.staging = staging; a.sizes = sizes;
    a.c16 = g_c16;
    return a;
}

// a coder launch as selected, on plane scratch of the size the selection asks for (poisoned: the decoder parks its
// finished planes there, planes above a codeblock's MSB are never written)
static void emu_bpc_launch(const BpcLaunch &l, BpcArgs &a)
{
    std::vector<uint32_t> plane_scratch(l.scratch_dwords, 0xDEADBEEFu);
    a.plane_scratch = plane_scratch.data();
    emu::launch(dim3(l.wgs), dim3(l.threads), [&] { l.kernel(a); });
}
// the decoder reading the packed stream itself: lengths + offsets out of it (scan_stream_kernel), the codewords at
// BpcArgs::cw16; `stream` holds stream_shorts shorts (a load may start at the last pair).  Returns the damaged-lengths flag.
static int emu_decode_from_stream(BpcArgs &a, const uint16_t *stream, unsigned stream_shorts, bool compact, bool c16)
{
    const int ncb = a.nCB;
    std::vector<int32_t> sizes(ncb), offsets(ncb);
    int32_t total = 0;
    int bad = 0;
    emu::launch(dim3(1), dim3(scan_threads(ncb)), [&] { scan_stream_kernel(stream, ncb, sizes.data(), offsets.data(), &total, &bad, 0); });
    a.sizes = sizes.data();
    a.cw16 = stream; a.cw16_offsets = offsets.data(); a.cw16_total = &total; a.cw16_max = stream_shorts;
    emu_bpc_launch(select_decoder(false, a.k > 0.0f, compact, true, c16, (unsigned)((ncb + 1) / 2)), a);
    return bad;
}

// what picsong_ctx_set_lut_component / _device decide about a table before a context takes it (lut_refusal): 0 = the
// context takes it, 1 = refused, the reason in msg
extern "C" int emu_lut_refusal(const int *geo, int wl, float k, int cp, int n_tables, char *msg, int cap)
{
    return lut_refusal(lut_geo(geo), wl, k > 0.0f, cp == 3, n_tables, msg, (size_t)cap) ? 1 : 0;
}

// codeblocks [cb_begin, cb_begin + cb_count) of the frame (cb_count < 0: all), like bpc_encode_impl
void emu_bpc_encode_range(const void *coeffs, int is_float, int aw, int ah, int wl, const int32_t *lut, const int *geo,
                          int32_t *staging, int32_t *sizes, int *flag, int cb_begin, int cb_count)
{
    BpcArgs a = mk(aw, ah, wl, lut, geo, nullptr, sizes, flag);
    a.coeffs_in = coeffs; a.is_float = is_float;
    a.k = 0.0f; a.n_tables = 1;
    if (cb_count < 0) cb_count = a.nCB - cb_begin;
    std::vector<uint16_t> st16((size_t)a.nCB * 4096, 0xDEADu);        // the encoders' 16-bit staging, poisoned
    a.staging16 = st16.data();
    a.cb_base = cb_begin; a.nCB = cb_begin + cb_count;
    emu_bpc_launch(select_encoder(false, false, false, (unsigned)((cb_count + 1) / 2)), a);
    // (as picsong_bpc_encode: widened into the caller's int32 array, words 0 .. len - 1 of the range's codeblocks)
    emu::launch(dim3((unsigned)cb_count), dim3(256), [&] { widen_staging_kernel(st16.data(), sizes, cb_begin, staging); });
}

// k > 0 (n_tables bit-plane tables in lut) runs the BULK instantiations, a pipelined context's (compact copies where
// the geometry allows them)
void emu_bpc_encode(const void *coeffs, int is_float, int aw, int ah, int wl, const int32_t *lut, const int *geo,
                    int32_t *staging, int32_t *sizes, int *flag, float k, int n_tables)
{
    BpcArgs a = mk(aw, ah, wl, lut, geo, nullptr, sizes, flag);
    a.coeffs_in = coeffs; a.is_float = is_float;
    a.k = k; a.n_tables = n_tables;
    std::vector<uint16_t> st16((size_t)a.nCB * 4096, 0xDEADu);
    a.staging16 = st16.data();
    memset(staging, 0xFF, (size_t)aw * ah * 4);
    emu_bpc_launch(select_encoder(false, k > 0.0f, k > 0.0f && emu_bulk_compact(aw, ah, wl, geo), (unsigned)((a.nCB + 1) / 2)), a);
    emu::launch(dim3((unsigned)a.nCB), dim3(256), [&] { widen_staging_kernel(st16.data(), sizes, 0, staging); });
}

void emu_bpc_decode(const int32_t *staging, const int32_t *sizes, int aw, int ah, int wl, const int32_t *lut,
                    const int *geo, int32_t *coeffs, int *flag, float k, int n_tables)
{
    BpcArgs a = mk(aw, ah, wl, lut, geo, const_cast<int32_t *>(staging), const_cast<int32_t *>(sizes), flag);
    a.coeffs_out = coeffs;
    a.k = k; a.n_tables = n_tables;
    const bool compact = k > 0.0f && emu_bulk_compact(aw, ah, wl, geo);
    emu_bpc_launch(select_decoder(false, k > 0.0f, compact, false, false, (unsigned)((a.nCB + 1) / 2)), a);
}

// the frame paths' decoder, k = 0 (emu_decode_from_stream)
int emu_bpc_decode_stream(const uint16_t *stream, unsigned stream_shorts, int aw, int ah, int wl, const int32_t *lut,
                          const int *geo, int32_t *coeffs, int *flag)
{
    BpcArgs a = mk(aw, ah, wl, lut, geo, nullptr, nullptr, flag);
    a.coeffs_out = coeffs;
    a.k = 0.0f; a.n_tables = 1;
    return emu_decode_from_stream(a, stream, stream_shorts, false, false);
}

// -k > 0 from the packed stream (both plane-count classes over the grid); c16: `coeffs` is an int16 Mallat array (the
// C16 instantiations)
int emu_bpc_decode_stream_k(const uint16_t *stream, unsigned stream_shorts, int aw, int ah, int wl, const int32_t *lut,
                            const int *geo, int32_t *coeffs, int *flag, float k, int n_tables, int c16)
{
    BpcArgs a = mk(aw, ah, wl, lut, geo, nullptr, nullptr, flag);
    a.coeffs_out = coeffs;
    a.k = k; a.n_tables = n_tables;
    return emu_decode_from_stream(a, stream, stream_shorts, emu_bulk_compact(aw, ah, wl, geo), c16 != 0);
}

// k = 0, the coefficients leaving as an int16 Mallat array (bpc_decode_kernel's C16 form)
int emu_bpc_decode_stream16(const uint16_t *stream, unsigned stream_shorts, int aw, int ah, int wl, const int32_t *lut,
                            const int *geo, int16_t *coeffs16, int *flag)
{
    BpcArgs a = mk(aw, ah, wl, lut, geo, nullptr, nullptr, flag);
    a.coeffs_out = reinterpret_cast<int32_t *>(coeffs16);
    a.k = 0.0f; a.n_tables = 1;
    return emu_decode_from_stream(a, stream, stream_shorts, false, true);
}

// -cp 3: geo[6..8] = nRef, nSig, nSign; lut = [ref | sig | sign | cp_sig | cp_sign]
void emu_bpc3_encode(const void *coeffs, int is_float, int aw, int ah, int wl, const int32_t *lut, const int *geo,
                     int32_t *staging, int32_t *sizes, int *flag)
{
    BpcArgs a = mk(aw, ah, wl, lut, geo, nullptr, sizes, flag);
    a.coeffs_in = coeffs; a.is_float = is_float; a.n_tables = 1;
    std::vector<uint16_t> st16((size_t)a.nCB * 4096, 0xDEADu);
    a.staging16 = st16.data();
    memset(staging, 0xFF, (size_t)aw * ah * 4);
    emu_bpc_launch(select_encoder(true, false, false, (unsigned)((a.nCB + 1) / 2)), a);
    emu::launch(dim3((unsigned)a.nCB), dim3(256), [&] { widen_staging_kernel(st16.data(), sizes, 0, staging); });
}

void emu_bpc3_decode(const int32_t *staging, const int32_t *sizes, int aw, int ah, int wl, const int32_t *lut,
                     const int *geo, int32_t *coeffs, int *flag)
{
    BpcArgs a = mk(aw, ah, wl, lut, geo, const_cast<int32_t *>(staging), const_cast<int32_t *>(sizes), flag);
    a.coeffs_out = coeffs; a.n_tables = 1;
    emu_bpc_launch(select_decoder(true, false, false, false, false, (unsigned)((a.nCB + 1) / 2)), a);
}

int emu_pack(const int32_t *staging, const int32_t *sizes, int ncb, const uint16_t *header, uint16_t *out)
{
    std::vector<int32_t> offsets(ncb);
    int32_t total = 0;
    HeaderArg h;
    memset(&h, 0, sizeof h);
    if (header) { memcpy(h.h, header, sizeof h.h); h.has = 1; }
    emu::launch(dim3(1), dim3(scan_threads(ncb)), [&] { scan_sizes_kernel(sizes, ncb, offsets.data(), &total); });
    emu::launch(dim3(pack_blocks<int32_t>(ncb)), dim3(256), [&] { pack_kernel<int32_t>(staging, sizes, offsets.data(), &total, ncb, h, out); });
    return total;
}

// the same from the encoders' 16-bit staging (the frame paths' pack)
int emu_pack16(const uint16_t *staging16, const int32_t *sizes, int ncb, const uint16_t *header, uint16_t *out)
{
    std::vector<int32_t> offsets(ncb);
    int32_t total = 0;
    HeaderArg h;
    memset(&h, 0, sizeof h);
    if (header) { memcpy(h.h, header, sizeof h.h); h.has = 1; }
    emu::launch(dim3(1), dim3(scan_threads(ncb)), [&] { scan_sizes_kernel(sizes, ncb, offsets.data(), &total); });
    emu::launch(dim3(pack_blocks<uint16_t>(ncb)), dim3(256), [&] { pack_kernel<uint16_t>(staging16, sizes, offsets.data(), &total, ncb, h, out); });
    return total;
}

int emu_unpack(const uint16_t *stream, int ncb, int32_t *staging, int32_t *sizes)
{
    std::vector<int32_t> offsets(ncb);
    int32_t total = 0;
    int flag = 0;
    memset(staging, 0xFF, (size_t)ncb * 4096 * 4);
    emu::launch(dim3((unsigned)((ncb + 255) / 256)), dim3(256), [&] { read_sizes_kernel(stream, ncb, sizes, &flag); });
    emu::launch(dim3(1), dim3(scan_threads(ncb)), [&] { scan_sizes_kernel(sizes, ncb, offsets.data(), &total); });
    emu::launch(dim3((unsigned)ncb), dim3(256), [&] { unpack_kernel(stream, sizes, offsets.data(), ncb, staging); });
    return flag;
}

}  // extern "C"
