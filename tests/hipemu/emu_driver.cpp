// TEST INFRASTRUCTURE ONLY -- runs the product's kernel sources on the CPU wave emulator and
// exposes host-memory entry points (ctypes) so tests can compare them with the oracle without a
// GPU.  The launch sequences (launch_seq.hpp), the plans (launch_plan.hpp) and the choice of kernel, grid and scratch
// (kernel_select.hpp) are the library's own, run through the emulator's launcher (emu::Go); what is written here is
// what picsong_hip.hip keeps in a context: buffers (poisoned), switches, and the return bits the tests read.
#include <hip/hip_runtime.h>

#include "../../cuda-image-and-video-codec_amd/csrc/launch_seq.hpp"

#include <string>

using namespace picsong;

// The launcher of this driver, in the idiom of CountGo (emu_decode_ctx.hpp): it notes WHICH kernel it is handed before it
// forwards to emu::Go.  The log keeps every distinct function pointer once, in the order of its first launch, so that a
// whole suite's launches do not grow it; tests/test_dwt_bands.py reads it against emu_dwt_selector_kernels.
static std::vector<const void *> g_launch_log;
struct RecordGo {
    template <typename K, typename... A>
    int operator()(K k, dim3 grid, unsigned threads, const A &...args) const
    {
        const void *p = reinterpret_cast<const void *>(k);
        bool seen = false;
        for (const void *q : g_launch_log) seen = seen || q == p;
        if (!seen) g_launch_log.push_back(p);
        return emu::Go{}(k, grid, threads, args...);
    }
};
static const RecordGo go{};
extern "C" void emu_launch_log_reset(void) { g_launch_log.clear(); }
// the distinct kernels launched since the reset: the first `cap` of them into ptrs, their number returned
extern "C" int emu_launch_log_read(const void **ptrs, int cap)
{
    for (int i = 0; i < cap && i < (int)g_launch_log.size(); i++) ptrs[i] = g_launch_log[(size_t)i];
    return (int)g_launch_log.size();
}

// what picsong_ctx_create decides once per context (cached here per (qs, wl))
static bool emu_fast_div(int lossy, float qs, int wl)
{
    static float c_qs = -1.0f;
    static int c_wl = -1;
    static bool c_ok = false;
    if (!lossy) return false;
    // (what the switch forces is not cached: a later call without it at the same qs and wl takes its own verdict)
    if (getenv("PICSONG_DWT_EXACTDIV")) return dequant_fast_ok(qs, wl);
    if (qs != c_qs || wl != c_wl) { c_ok = dequant_fast_ok(qs, wl); c_qs = qs; c_wl = wl; }
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

// frame paths: coded coefficients as int16 (DwtFwdArgs::c16 / BpcArgs::c16), switched on by the tests
static int g_c16 = 0;
extern "C" void emu_set_c16(int on) { g_c16 = on; }
extern "C" int emu_coef16_ok(int lossy, int wl, float qs, int in_max, int aw, int ah)
{
    return coef16_ok(lossy != 0, wl, qs, in_max) && dwt_c16_geometry_ok(aw, ah, wl) ? 1 : 0;
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

// Host only, the twin of emu_dwt_vec_levels: what the plans choose per level under the current environment, out[2 l] =
// the band height of level l and out[2 l + 1] = its vec flag, for plan_dwt_forward (u8 input) and for plan_dwt_inverse
// (`fast`: the context's verified reciprocal divisions, 9/7 only -- what sends the plan to inv97_band_rows).  The plans
// see 64-byte aligned pointers and dereference nothing.
void emu_dwt_plan_bands(int aw, int ah, int wl, int lossy, int fast, int *out_fwd, int *out_inv)
{
    const void *in = (const void *)(uintptr_t)4096;
    void *out = (void *)(uintptr_t)8192;
    for (const FwdLaunch &f : plan_dwt_forward(in, true, out, aw, ah, wl, 1.0f)) {
        out_fwd[2 * f.a.level] = f.band; out_fwd[2 * f.a.level + 1] = f.vec ? 1 : 0;
    }
    int l = wl - 1;
    for (const InvLaunch &f : plan_dwt_inverse((const int32_t *)in, out, aw, ah, wl, 1.0f, lossy != 0 && fast != 0)) {
        out_inv[2 * l] = f.band; out_inv[2 * l + 1] = f.vec ? 1 : 0;
        l--;
    }
}

// Host only: every kernel select_fwd, select_inv and select_inv_rgb (kernel_select.hpp) can return for a launch the plans
// can form -- band 4 / 8 / 16 / 32; vec, u8, lossy; fast, lean97, c16, dst_u8, first, one_div.  What the plans never
// form is left out: the 16-bit form and the pixel store off the vector kernels (plan_dwt_inverse, plan_inverse_frames),
// fast without lossy, 9/7 16-bit coefficients without the verified divisions or on the coarsest level that also writes
// pixels (dec_c16_ok).  The distinct pointers into ptrs, a label each (the first combination that gave it) into labels +
// i * label_bytes; returns their number (beyond cap: counted, not written).
int emu_dwt_selector_kernels(const void **ptrs, char *labels, int label_bytes, int cap)
{
    std::vector<const void *> seen;
    auto add = [&](const void *p, const std::string &label) {
        for (const void *q : seen) if (q == p) return;
        if ((int)seen.size() < cap) {
            ptrs[seen.size()] = p;
            snprintf(labels + seen.size() * (size_t)label_bytes, (size_t)label_bytes, "%s", label.c_str());
        }
        seen.push_back(p);
    };
    auto s = [](const char *name, int v) { return std::string(" ") + name + "=" + std::to_string(v); };
    static uint8_t pixel;
    const int bands[4] = { 4, 8, 16, 32 };
    for (int band : bands)
        for (int lossy = 0; lossy < 2; lossy++) {
            for (int vec = 0; vec < 2; vec++)
                for (int u8 = 0; u8 < 2; u8++) {
                    FwdLaunch f;
                    memset(&f, 0, sizeof f);
                    f.band = band; f.vec = vec != 0; f.u8 = u8 != 0;
                    add(reinterpret_cast<const void *>(select_fwd(lossy != 0, f)), "fwd" + s("band", band) + s("lossy", lossy) + s("vec", vec) + s("u8", u8));
                }
            for (int bits = 0; bits < 128; bits++) {
                const int vec = bits & 1, fast = (bits >> 1) & 1, lean97 = (bits >> 2) & 1, c16 = (bits >> 3) & 1;
                const int u8out = (bits >> 4) & 1, first = (bits >> 5) & 1, one_div = (bits >> 6) & 1;
                if ((c16 || u8out) && !vec) continue;
                if (fast && !lossy) continue;
                if (c16 && ((lossy && !(fast && lean97)) || (first && u8out))) continue;
                InvLaunch f;
                memset(&f, 0, sizeof f);
                f.band = band; f.vec = vec != 0; f.fast = fast != 0;
                f.a.c16 = c16; f.a.first = first; f.a.one_div = one_div; f.a.dst_u8 = u8out ? &pixel : nullptr;
                add(reinterpret_cast<const void *>(select_inv(lossy != 0, lean97 != 0, f)),
                    "inv" + s("band", band) + s("lossy", lossy) + s("vec", vec) + s("fast", fast) + s("lean97", lean97) + s("c16", c16) +
                        s("dst_u8", u8out) + s("first", first) + s("one_div", one_div));
            }
            for (int one_div = 0; one_div < 2; one_div++) {
                InvLaunch f;
                memset(&f, 0, sizeof f);
                f.band = band; f.vec = true; f.fast = lossy != 0; f.a.c16 = 1; f.a.one_div = one_div; f.a.W = 64;
                add(reinterpret_cast<const void *>(select_inv_rgb(lossy != 0, f).kernel), "inv_rgb" + s("band", band) + s("lossy", lossy) + s("one_div", one_div));
            }
        }
    return (int)seen.size();
}

// as dwt_forward_impl (picsong_hip.hip); returns 1 when levels 0 and 1 went through the fused kernel
int emu_dwt_forward(const void *in, int u8in, void *out, int aw, int ah, int wl, int lossy, float qs)
{
    bool fused01 = false;
    launch_fwd_plan(go, lossy != 0, plan_dwt_forward(in, u8in != 0, out, aw, ah, wl, qs, g_c16 != 0), 1, &fused01);
    return fused01 ? 1 : 0;
}

// picsong_encode_rgb_frame's transform (rgb_forward_transform; out: three coefficient buffers of `stride` bytes, int16
// Mallat arrays at their starts); returns 1 when the fused form applies: the colour transform (RCT / ICT) in the fused
// head's load stage, one launch for the three components
int emu_dwt_forward_rgb(const uint8_t *r, const uint8_t *g, const uint8_t *b, void *out, size_t stride, int aw, int ah, int wl,
                        int lossy, float qs)
{
    const size_t P = (size_t)aw * ah;
    std::vector<int32_t> planes(3 * P);
    auto plan_of = [&](const void *src, bool u8in) { return plan_dwt_forward(src, u8in, out, aw, ah, wl, qs, true); };
    bool fused = false;
    rgb_forward_transform(go, lossy != 0, true, plan_of, true, r, g, b, planes.data(), P, 128, stride, nullptr, &fused);
    return fused ? 1 : 0;
}
// the same call where the fused head may refuse (PICSONG_DWT_NOFUSE01=1: the colour transform on its own, then every
// level of the three components through dwt_fwd_kernel); returns bit 0: the fused form ran, bit 1: the coefficients
// left as int16 Mallat arrays (else: 32-bit ones at the same places)
int emu_dwt_forward_rgb_forms(const uint8_t *r, const uint8_t *g, const uint8_t *b, void *out, size_t stride, int aw, int ah, int wl,
                              int lossy, float qs)
{
    const size_t P = (size_t)aw * ah;
    std::vector<int32_t> store(3 * P + 16);
    int32_t *const planes = (int32_t *)(((uintptr_t)store.data() + 63) & ~(uintptr_t)63);
    auto plan_of = [&](const void *src, bool u8in) { return plan_dwt_forward(src, u8in, out, aw, ah, wl, qs, true); };
    bool fused = false, c16 = false;
    rgb_forward_transform(go, lossy != 0, true, plan_of, true, r, g, b, planes, P, 128, stride, &c16, &fused);
    return (fused ? 1 : 0) | (c16 ? 2 : 0);
}

// picsong_dwt_forward_band / picsong_dwt_forward_tail
void emu_dwt_forward_band(const void *in, void *out, int aw, int ah, int wl, int lossy, float qs, int row0, int rows)
{
    std::vector<FwdLaunch> plan = plan_dwt_forward(in, true, out, aw, ah, wl, qs);
    plan_restrict_band(plan[0], row0, rows);
    plan.resize(1);
    launch_fwd_levels(go, lossy != 0, plan, 0);
}

void emu_dwt_forward_tail(void *out, int aw, int ah, int wl, int lossy, float qs)
{
    launch_fwd_levels(go, lossy != 0, plan_dwt_forward(out, false, out, aw, ah, wl, qs), 1);
}

void emu_dwt_inverse(const int32_t *in, void *out, int aw, int ah, int wl, int lossy, float qs)
{
    run_inverse(go, lossy != 0, emu_lean97(), plan_dwt_inverse(in, out, aw, ah, wl, qs, emu_fast_div(lossy, qs, wl)));
}

// the frame paths' synthesis plan (inverse_plan, picsong_hip.hip); no pixels: an RGB frame's components (planes_out)
static std::vector<InvLaunch> emu_inverse_plan(const void *in, void *scratch, uint8_t *pixels, bool *fused, unsigned frames,
                                               bool c16, int aw, int ah, int wl, float qs, bool fast, size_t P, size_t extra)
{
    return plan_inverse_frames((const int32_t *)in, scratch, pixels, fused, frames, 0, c16, pixels == nullptr, 0, aw, ah, wl, qs, fast,
                               128, P, extra);
}

// the frame path's inverse: the finest level writes clamped pixels (inverse_plan + run_inverse, 32-bit coefficients);
// returns 1 when that fused kernel applied
int emu_dwt_inverse_u8(const int32_t *in, void *scratch, uint8_t *pixels, int aw, int ah, int wl, int lossy, float qs)
{
    bool fused = false;
    run_inverse(go, lossy != 0, emu_lean97(), emu_inverse_plan(in, scratch, pixels, &fused, 1, false, aw, ah, wl, qs,
                                                                emu_fast_div(lossy, qs, wl), (size_t)aw * ah, dwt_extra(aw, ah, wl)));
    return fused ? 1 : 0;
}

// `frames` frames a call, grid.z = frame (picsong_encode_frames / picsong_decode_frames): frame z's input in_z bytes and
// its coefficient buffer out_z bytes after frame z - 1's; returns 1 when levels 0 and 1 went through the fused kernel
int emu_dwt_forward_n(const void *in, int u8in, unsigned long long in_z, void *out, unsigned long long out_z, int aw, int ah, int wl,
                      int lossy, float qs, int frames)
{
    std::vector<FwdLaunch> plan = plan_dwt_forward(in, u8in != 0, out, aw, ah, wl, qs, g_c16 != 0);
    plan_frame_strides(plan, in_z, out_z);
    bool fused01 = false;
    launch_fwd_plan(go, lossy != 0, plan, (unsigned)frames, &fused01);
    return fused01 ? 1 : 0;
}
// ... frame z's 32-bit coefficients P words, its scratch P + extra words, its pixels P bytes after frame z - 1's; returns 1
// when the finest level wrote the pixels (else nothing in `pixels` is defined)
int emu_dwt_inverse_u8_n(const int32_t *in, void *scratch, uint8_t *pixels, int aw, int ah, int wl, int lossy, float qs, int frames)
{
    bool fused = false;
    const size_t P = (size_t)aw * ah;
    run_inverse(go, lossy != 0, emu_lean97(),
                plan_inverse_frames(in, scratch, pixels, &fused, (unsigned)frames, P, false, false, 0, aw, ah, wl, qs,
                                    emu_fast_div(lossy, qs, wl), 128, P, dwt_extra(aw, ah, wl)),
                (unsigned)frames);
    return fused ? 1 : 0;
}

// the decode frame paths with 16-bit coefficients (inverse_plan + run_inverse, picsong_hip.hip): `in16` is an
// int16 Mallat array; returns bit 0: the finest level wrote the pixels, bit 1: levels 1 and 0 ran as ONE launch
// (dwt_inv2_kernel), bit 2: the plan took the 16-bit form (0: the caller's geometry / context does not allow it)
int emu_dwt_inverse_u8_c16(const int16_t *in16, void *scratch, uint8_t *pixels, int aw, int ah, int wl, int lossy, float qs)
{
    const bool fast = emu_fast_div(lossy, qs, wl);
    if (!dec_c16_ok(lossy != 0, wl, qs, 128, aw, ah, fast)) return 0;
    bool px = false, fused10 = false;
    const std::vector<InvLaunch> plan = emu_inverse_plan(in16, scratch, pixels, &px, 1, true, aw, ah, wl, qs, fast, (size_t)aw * ah,
                                                         dwt_extra(aw, ah, wl));
    if (!plan_inv_is_c16(plan)) return 0;
    run_inverse(go, lossy != 0, emu_lean97(), plan, 1, &fused10);
    return 4 | (px ? 1 : 0) | (fused10 ? 2 : 0);
}

// picsong_decode_rgb_frame's synthesis with 16-bit coefficients (run_inverse_rgb): the levels above the finest, grid.z =
// component, then the finest level of all three components + the inverse colour transform as ONE launch.
// in16: three int16 Mallat arrays in_z = 2 P BYTES apart; scratch: three work buffers wrk_z = 4 (P + extra) bytes apart.
// Returns 1 when the form applies.
int emu_dwt_inverse_rgb(const int16_t *in16, size_t in_z, void *scratch, size_t wrk_z, uint8_t *r, uint8_t *g, uint8_t *b,
                        int aw, int ah, int wl, int lossy, float qs)
{
    const bool fast = emu_fast_div(lossy, qs, wl);
    if (!dec_c16_ok(lossy != 0, wl, qs, 255, aw, ah, fast)) return 0;
    const std::vector<InvLaunch> plan = emu_inverse_plan(in16, scratch, nullptr, nullptr, 3u, true, aw, ah, wl, qs, fast, in_z / 2,
                                                         wrk_z / 4 - in_z / 2);
    if (!inv_rgb_tail_ok(plan, lossy != 0)) return 0;
    run_inverse_rgb(go, lossy != 0, emu_lean97(), plan, 128, r, g, b);
    return 1;
}

void emu_level_shift_inv(void *data, size_t n, int lossy) { level_shift_inv(go, lossy != 0, data, n, 128); }
void emu_clamp_to_u8(const void *data, uint8_t *out, size_t n, int lossy) { clamp_pixels(go, lossy != 0, data, out, n / 4, 128); }
void emu_level_shift_fwd(const uint8_t *in, void *out, size_t n, int lossy) { level_shift_fwd(go, lossy != 0, in, out, n / 4, 128); }
void emu_rgb_forward(const uint8_t *r, const uint8_t *g, const uint8_t *b, void *c0, void *c1, void *c2, size_t n, int lossy)
{
    rgb_forward(go, lossy != 0, r, g, b, c0, c1, c2, n / 4, 128);
}
void emu_rgb_inverse(const void *c0, const void *c1, const void *c2, uint8_t *r, uint8_t *g, uint8_t *b, size_t n, int lossy)
{
    rgb_inverse(go, lossy != 0, c0, c1, c2, r, g, b, n / 4, 128);
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

// An encoder launch over codeblocks [cb_begin, cb_begin + cb_count) on 16-bit staging and plane scratch of the size the
// selection asks for (both poisoned), then, as picsong_bpc_encode, widened into the caller's int32 array
static void emu_encode_widened(BpcArgs &a, bool cp3, bool compact, int cb_begin, int cb_count, int32_t *staging)
{
    const unsigned waves = (unsigned)((cb_count + 1) / 2);
    std::vector<uint16_t> st16((size_t)a.nCB * 4096, 0xDEADu);
    std::vector<uint32_t> plane_scratch(encoder_scratch_dwords(cp3, a.k > 0.0f, waves), 0xDEADBEEFu);
    a.staging16 = st16.data(); a.plane_scratch = plane_scratch.data();
    a.cb_base = cb_begin; a.nCB = cb_begin + cb_count;
    launch_encoder(go, a, cp3, compact, waves);
    widen_staging(go, st16.data(), a.sizes, cb_begin, cb_count, staging);
}
// A decoder launch over the frame on poisoned plane scratch (the decoder parks its finished planes there, planes above
// a codeblock's MSB are never written), from a.staging / a.sizes -- or, stream != nullptr, reading the packed stream
// itself: lengths + offsets out of it (stream_intake), the codewords at BpcArgs::cw16; `stream` holds stream_shorts
// shorts (a load may start at the last pair).  Returns the damaged-lengths flag.
static int emu_decode(BpcArgs &a, bool cp3, bool compact, int32_t *coeffs, const uint16_t *stream = nullptr,
                      unsigned stream_shorts = 0, bool c16 = false)
{
    const int ncb = a.nCB;
    const unsigned waves = (unsigned)((ncb + 1) / 2);
    std::vector<int32_t> sizes(ncb), offsets(ncb);
    std::vector<uint32_t> plane_scratch(decoder_scratch_dwords(cp3, a.k > 0.0f, waves), 0xDEADBEEFu);
    int32_t total = 0;
    int bad = 0;
    const Workspace w = { nullptr, a.staging, stream ? sizes.data() : a.sizes, offsets.data(), &total, plane_scratch.data(), coeffs };
    if (stream) stream_intake(go, stream, 1u, 0, true, ncb, 0, w, &bad);
    launch_decoder(go, a, cp3, waves, compact, w, stream, 0, stream_shorts, c16);
    return bad;
}
// scan + pack of one frame's codeblocks; returns the stream's length
extern "C++" template <typename W>
int emu_pack_frame(const W *staging, const int32_t *sizes, int ncb, const uint16_t *header, uint16_t *out)
{
    std::vector<int32_t> offsets(ncb);
    int32_t total = 0;
    const Workspace w = { nullptr, nullptr, const_cast<int32_t *>(sizes), offsets.data(), &total, nullptr, nullptr };
    pack_frames(go, staging, w, ncb, 1u, header, 1, out, 0, 0);
    return total;
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
    emu_encode_widened(a, false, false, cb_begin, cb_count, staging);
}

// k > 0 (n_tables bit-plane tables in lut) runs the BULK instantiations, a pipelined context's (compact copies where
// the geometry allows them)
void emu_bpc_encode(const void *coeffs, int is_float, int aw, int ah, int wl, const int32_t *lut, const int *geo,
                    int32_t *staging, int32_t *sizes, int *flag, float k, int n_tables)
{
    BpcArgs a = mk(aw, ah, wl, lut, geo, nullptr, sizes, flag);
    a.coeffs_in = coeffs; a.is_float = is_float;
    a.k = k; a.n_tables = n_tables;
    memset(staging, 0xFF, (size_t)aw * ah * 4);
    emu_encode_widened(a, false, k > 0.0f && emu_bulk_compact(aw, ah, wl, geo), 0, a.nCB, staging);
}

void emu_bpc_decode(const int32_t *staging, const int32_t *sizes, int aw, int ah, int wl, const int32_t *lut,
                    const int *geo, int32_t *coeffs, int *flag, float k, int n_tables)
{
    BpcArgs a = mk(aw, ah, wl, lut, geo, const_cast<int32_t *>(staging), const_cast<int32_t *>(sizes), flag);
    a.k = k; a.n_tables = n_tables;
    emu_decode(a, false, k > 0.0f && emu_bulk_compact(aw, ah, wl, geo), coeffs);
}

// the frame paths' decoder, k = 0 (emu_decode from the stream)
int emu_bpc_decode_stream(const uint16_t *stream, unsigned stream_shorts, int aw, int ah, int wl, const int32_t *lut,
                          const int *geo, int32_t *coeffs, int *flag)
{
    BpcArgs a = mk(aw, ah, wl, lut, geo, nullptr, nullptr, flag);
    a.k = 0.0f; a.n_tables = 1;
    return emu_decode(a, false, false, coeffs, stream, stream_shorts);
}

// -k > 0 from the packed stream (both plane-count classes over the grid); c16: `coeffs` is an int16 Mallat array (the
// C16 instantiations)
int emu_bpc_decode_stream_k(const uint16_t *stream, unsigned stream_shorts, int aw, int ah, int wl, const int32_t *lut,
                            const int *geo, int32_t *coeffs, int *flag, float k, int n_tables, int c16)
{
    BpcArgs a = mk(aw, ah, wl, lut, geo, nullptr, nullptr, flag);
    a.k = k; a.n_tables = n_tables;
    return emu_decode(a, false, emu_bulk_compact(aw, ah, wl, geo), coeffs, stream, stream_shorts, c16 != 0);
}

// k = 0, the coefficients leaving as an int16 Mallat array (bpc_decode_kernel's C16 form)
int emu_bpc_decode_stream16(const uint16_t *stream, unsigned stream_shorts, int aw, int ah, int wl, const int32_t *lut,
                            const int *geo, int16_t *coeffs16, int *flag)
{
    BpcArgs a = mk(aw, ah, wl, lut, geo, nullptr, nullptr, flag);
    a.k = 0.0f; a.n_tables = 1;
    return emu_decode(a, false, false, reinterpret_cast<int32_t *>(coeffs16), stream, stream_shorts, true);
}

// -cp 3: geo[6..8] = nRef, nSig, nSign; lut = [ref | sig | sign | cp_sig | cp_sign]
void emu_bpc3_encode(const void *coeffs, int is_float, int aw, int ah, int wl, const int32_t *lut, const int *geo,
                     int32_t *staging, int32_t *sizes, int *flag)
{
    BpcArgs a = mk(aw, ah, wl, lut, geo, nullptr, sizes, flag);
    a.coeffs_in = coeffs; a.is_float = is_float; a.n_tables = 1;
    memset(staging, 0xFF, (size_t)aw * ah * 4);
    emu_encode_widened(a, true, false, 0, a.nCB, staging);
}

void emu_bpc3_decode(const int32_t *staging, const int32_t *sizes, int aw, int ah, int wl, const int32_t *lut,
                     const int *geo, int32_t *coeffs, int *flag)
{
    BpcArgs a = mk(aw, ah, wl, lut, geo, const_cast<int32_t *>(staging), const_cast<int32_t *>(sizes), flag);
    a.n_tables = 1;
    emu_decode(a, true, false, coeffs);
}

int emu_pack(const int32_t *staging, const int32_t *sizes, int ncb, const uint16_t *header, uint16_t *out)
{
    return emu_pack_frame(staging, sizes, ncb, header, out);
}

// the same from the encoders' 16-bit staging (the frame paths' pack)
int emu_pack16(const uint16_t *staging16, const int32_t *sizes, int ncb, const uint16_t *header, uint16_t *out)
{
    return emu_pack_frame(staging16, sizes, ncb, header, out);
}

int emu_unpack(const uint16_t *stream, int ncb, int32_t *staging, int32_t *sizes)
{
    std::vector<int32_t> offsets(ncb);
    int32_t total = 0;
    int flag = 0;
    memset(staging, 0xFF, (size_t)ncb * 4096 * 4);
    const Workspace w = { nullptr, staging, sizes, offsets.data(), &total, nullptr, nullptr };
    stream_intake(go, stream, 1u, 0, false, ncb, 0, w, &flag);
    return flag;
}

}  // extern "C"
