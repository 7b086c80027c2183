// TEST INFRASTRUCTURE ONLY -- deep contexts (bit_depth 9..16, uint16 samples) on the CPU wave emulator: the library's own
// plans (plan_dwt_forward_u16, plan_inverse_frames with px_max), selectors (select_fwd / select_inv / select_ingest /
// select_emit) and launch sequences (deep_forward, decode_frames, launch_encoder, pack_frames, ingest_frames, emit_frames;
// launch_seq.hpp) over the kernel sources of cuda-image-and-video-codec_amd/csrc, through a launcher that records which
// kernels it was handed.  What a context keeps -- the buffers (poisoned), the tables, the switches -- is
// emu_decode_ctx.hpp's; PICSONG_DEEP_NOFUSE, PICSONG_DWT_BANDS and PICSONG_DWT_EXACTDIV are read at every call.
// Built by tests/test_deep_emulated.py with the flags of tests/hipemu/Makefile.
#include "emu_decode_ctx.hpp"

#include <string>

static std::vector<const void *> g_log;
struct RecordGo {
    template <typename K, typename... A>
    int operator()(K k, dim3 grid, unsigned threads, const A &...args) const
    {
        const void *p = reinterpret_cast<const void *>(k);
        bool seen = false;
        for (const void *q : g_log) seen = seen || q == p;
        if (!seen) g_log.push_back(p);
        return emu::Go{}(k, grid, threads, args...);
    }
};
static const RecordGo rgo{};

extern "C" {

void emu_deep_log_reset(void) { g_log.clear(); }
int emu_deep_log_read(const void **ptrs, int cap)
{
    for (int i = 0; i < cap && i < (int)g_log.size(); i++) ptrs[i] = g_log[(size_t)i];
    return (int)g_log.size();
}

// Host only: every kernel the selectors can return for a DEEP launch -- select_fwd with FwdLaunch::u16 (band, vec, lossy),
// select_inv with DwtInvArgs::dst_u16 (band; 5/3, 9/7 dividing, 9/7 FAST; the lean97 switch must not matter), the GREY16
// layout kernels (ingest / emit, vector and per-sample).  The distinct pointers into ptrs, a label each; their number.
int emu_deep_selector_kernels(const void **ptrs, char *labels, int label_bytes, int cap)
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
    static uint16_t sample;
    const int bands[4] = { 4, 8, 16, 32 };
    for (int band : bands)
        for (int lossy = 0; lossy < 2; lossy++) {
            for (int vec = 0; vec < 2; vec++) {
                FwdLaunch f;
                memset(&f, 0, sizeof f);
                f.band = band; f.vec = vec != 0; f.u16 = true;
                add(reinterpret_cast<const void *>(select_fwd(lossy != 0, f)), "fwd16" + s("band", band) + s("lossy", lossy) + s("vec", vec));
            }
            for (int fast = 0; fast <= lossy; fast++)
                for (int lean97 = 0; lean97 < 2; lean97++) {
                    InvLaunch f;
                    memset(&f, 0, sizeof f);
                    f.band = band; f.vec = true; f.fast = fast != 0; f.a.dst_u16 = &sample;
                    add(reinterpret_cast<const void *>(select_inv(lossy != 0, lean97 != 0, f)), "inv16" + s("band", band) + s("lossy", lossy) + s("fast", fast));
                }
        }
    for (int vec = 0; vec < 2; vec++) {
        LayoutArgs a;
        memset(&a, 0, sizeof a);
        a.img = (uint8_t *)(uintptr_t)(vec ? 4096 : 4098); a.pad = (uint8_t *)(uintptr_t)8192; a.pitch = 512;
        a.W = 200; a.H = 136; a.AW = 256; a.AH = 192;
        add(reinterpret_cast<const void *>(select_ingest(kLayoutGrey16, a).kernel), "ingest16" + s("vec", vec));
        add(reinterpret_cast<const void *>(select_emit(kLayoutGrey16, a).kernel), "emit16" + s("vec", vec));
    }
    return (int)seen.size();
}

// picsong_dwt_forward_u16 / the transform of picsong_encode_frames16: n frames of uint16 samples frame_stride bytes apart
// to n coefficient buffers of P + extra elements (coef: 16-byte aligned).  Returns bit 0: level 0 read the samples itself,
// bit 1: through its vector form.
int emu_deep_forward(const uint16_t *frames, unsigned long long frame_stride, int n, void *coef, int aw, int ah, int wl, int lossy, float qs, int bd)
{
    const size_t P = (size_t)aw * ah, extra = dwt_extra(aw, ah, wl);
    std::vector<int32_t> shifted((size_t)n * P + 16, 0x5A5A5A5A);
    void *const sh = (void *)(((uintptr_t)shifted.data() + 63) & ~(uintptr_t)63);
    bool in_kernel = false;
    if (deep_forward(rgo, lossy != 0, deep_nofuse(), frames, (size_t)frame_stride, (unsigned)n, coef, sh, aw, ah, wl, qs, 1 << (bd - 1),
                     (unsigned long long)(P + extra) * 4ull, &in_kernel)) return -1;
    const bool vec = in_kernel && plan_dwt_forward_u16(frames, n > 1 ? (size_t)frame_stride : 0, (unsigned)n, coef, aw, ah, wl, qs, 1 << (bd - 1))[0].vec;
    return (in_kernel ? 1 : 0) | (vec ? 2 : 0);
}

// The synthesis of picsong_decode_frames16 (decode_frames behind its decoder): n int32 Mallat arrays (16-byte aligned, P
// words each) to n frames of uint16 samples frame_stride bytes apart.  Returns bit 0: the finest level stored the samples.
int emu_deep_inverse(const int32_t *coef, uint16_t *out, unsigned long long frame_stride, int n, int aw, int ah, int wl, int lossy, float qs, int bd)
{
    const size_t P = (size_t)aw * ah, extra = dwt_extra(aw, ah, wl);
    std::vector<int32_t> work((size_t)n * (P + extra) + 16, 0x5A5A5A5A);
    void *const wrk = (void *)(((uintptr_t)work.data() + 63) & ~(uintptr_t)63);
    const bool fast = lossy && dequant_fast_ok(qs, wl);
    const int off = 1 << (bd - 1), mx = (1 << bd) - 1;
    bool fused = false;
    if (n <= 1) frame_stride = 0;
    const std::vector<InvLaunch> plan = plan_inverse_frames(coef, wrk, (uint8_t *)out, &fused, (unsigned)n, (size_t)frame_stride, false, false, 0,
                                                            aw, ah, wl, qs, fast, off, P, extra, mx);
    if (run_inverse(rgo, lossy != 0, true, plan, (unsigned)n)) return -1;
    for (int f = 0; f < n && !fused; f++)
        if (clamp_pixels16(rgo, lossy != 0, (const char *)plan.back().a.dst + (size_t)f * (P + extra) * 4,
                           (uint16_t *)((char *)out + (size_t)f * frame_stride), P / 4, off, mx)) return -1;
    return fused ? 1 : 0;
}

// the element-wise ends on their own (picsong_level_shift_fwd16, picsong_level_shift_inv on a deep context)
int emu_deep_level_shift_fwd(const uint16_t *in, void *out, size_t n4, int lossy, int bd)
{
    return level_shift_fwd16(rgo, lossy != 0, in, out, n4, 1 << (bd - 1));
}
int emu_deep_level_shift_inv(void *data, size_t n, int lossy, int bd)
{
    return level_shift_inv16(rgo, lossy != 0, data, n, 1 << (bd - 1), (1 << bd) - 1);
}

// picsong_encode_frames16: transform, coder (32-bit coefficients, one grid over the n frames), pack.  header: the nine
// populated shorts.  Out: the n streams stream_stride shorts apart, totals[n].  Returns -1: a launch failed; else
// emu_deep_forward's bits.
int emu_deep_encode(const uint16_t *frames, unsigned long long frame_stride, int n, int first_iter, uint16_t *streams,
                    unsigned long long stream_stride, int32_t *totals, int aw, int ah, int wl, int lossy, float qs, int bd, const int32_t *lut,
                    const int *geo, float k, int n_tables, const uint16_t *header, int *flag)
{
    const size_t P = (size_t)aw * ah, extra = dwt_extra(aw, ah, wl), coef_z = (P + extra) * 4;
    const int ncb = (aw / 64) * (ah / 64);
    std::vector<int32_t> coef((size_t)n * (P + extra) + 16, 0x5A5A5A5A);
    void *const cf = (void *)(((uintptr_t)coef.data() + 63) & ~(uintptr_t)63);
    const int bits = emu_deep_forward(frames, frame_stride, n, cf, aw, ah, wl, lossy, qs, bd);
    if (bits < 0) return -1;
    const int32_t *luts[3] = { lut, nullptr, nullptr };
    BpcArgs a = table_args(aw, ah, wl, luts, geo, k, n_tables, flag);
    const int wpf = (ncb + 1) / 2;
    const unsigned waves = (unsigned)n * (unsigned)wpf;
    std::vector<uint16_t> st16((size_t)n * P * 2, 0xDEADu);
    std::vector<int32_t> sizes((size_t)n * ncb, -7), offsets((size_t)n * ncb, -7);
    std::vector<uint32_t> scratch(encoder_scratch_dwords(false, k > 0.0f, waves), 0xDEADBEEFu);
    a.c16 = 0; a.cb_base = 0; a.nCB = ncb; a.coeffs_in = cf; a.is_float = lossy ? 1 : 0; a.coef_z = coef_z;
    a.staging16 = st16.data(); a.sizes = sizes.data(); a.plane_scratch = scratch.data();
    a.frames = n; a.waves_per_frame = wpf;
    if (launch_encoder(rgo, a, false, emu_compact(aw, ah, wl, geo, k), waves)) return -1;
    const Workspace w = { nullptr, nullptr, sizes.data(), offsets.data(), totals, nullptr, nullptr };
    const bool has0 = first_iter <= 0 && first_iter + n > 0;
    if (pack_frames(rgo, st16.data(), w, ncb, (unsigned)n, has0 ? header : nullptr, -first_iter + 1, streams, P, (size_t)stream_stride)) return -1;
    return bits;
}

// picsong_decode_frames16 under the context's `drop`: decode_frames with DecodeCtx::px_max.  Returns -1: a launch failed;
// else bit 0: the finest level stored the samples, bit 1: 16-bit coefficients (never), bit 3: the lengths were damaged.
int emu_deep_decode(const uint16_t *streams, unsigned long long stream_stride, int n, uint16_t *out, unsigned long long frame_stride, int aw,
                    int ah, int wl, int lossy, float qs, int bd, const int32_t *lut, const int *geo, float k, int n_tables, int drop, int *flag)
{
    Ctx c(n, false, aw, ah, wl, lossy, qs, lut, nullptr, nullptr, geo, k, n_tables, flag, (uint32_t)max_stream_shorts(aw, ah));
    c.g.off = 1 << (bd - 1); c.g.px_max = (1 << bd) - 1;
    c.a.drop = drop;
    DecodeReport rep;
    if (decode_frames(rgo, c.g, c.a, c.w, (unsigned)n, streams, (size_t)stream_stride, 0, nullptr, false, true, (uint8_t *)out,
                      (size_t)frame_stride, 0, &rep)) return -1;
    return (rep.pixels ? 1 : 0) | (rep.c16 ? 2 : 0) | (c.bad ? 8 : 0);
}

// GREY16 through picsong_ingest_frames / picsong_emit_frames: layout_refusal, then the sequences.  Returns -1: refused
// (the reason in msg), else bit 0: the vector form ran.
int emu_deep_ingest(const void *data, unsigned long long pitch, unsigned long long frame_stride, uint16_t *padded, unsigned long long padded_stride,
                    int n, int w, int h, int aw, int ah, char *msg, int cap)
{
    const char *why = layout_refusal(kLayoutGrey16, data, (size_t)pitch, 0, (size_t)frame_stride, padded, (size_t)padded_stride, n, w, h, aw, ah, true);
    if (msg && cap > 0) snprintf(msg, (size_t)cap, "%s", why ? why : "");
    if (why) return -1;
    bool vec = false;
    if (ingest_frames(rgo, kLayoutGrey16, data, (size_t)pitch, 0, (size_t)frame_stride, (uint8_t *)padded, (size_t)padded_stride, n, w, h, aw, ah, &vec)) return -1;
    return vec ? 1 : 0;
}
int emu_deep_emit(const uint16_t *padded, unsigned long long padded_stride, void *data, unsigned long long pitch, unsigned long long frame_stride,
                  int n, int w, int h, int aw, int ah, char *msg, int cap)
{
    const char *why = layout_refusal(kLayoutGrey16, data, (size_t)pitch, 0, (size_t)frame_stride, padded, (size_t)padded_stride, n, w, h, aw, ah, true);
    if (msg && cap > 0) snprintf(msg, (size_t)cap, "%s", why ? why : "");
    if (why) return -1;
    bool vec = false;
    if (emit_frames(rgo, kLayoutGrey16, (const uint8_t *)padded, (size_t)padded_stride, data, (size_t)pitch, 0, (size_t)frame_stride, n, w, h, aw, ah, &vec)) return -1;
    return vec ? 1 : 0;
}

}  // extern "C"
