// launch_seq.hpp -- the launch sequences of the frame pipeline (pure host code): which kernels a call launches, in what
// order, with what arguments wired between them, and which fused form it takes.  The one copy: the C-ABI implementation
// (picsong_hip.hip) and the CPU wave-emulator drivers (tests/hipemu/) both run these, each through its launcher
//     go(kernel, dim3 grid, unsigned threads, args...) -> int, 0 = ok
// -- the library's holds the stream and does kernel<<<grid, threads, 0, s>>>(args...), the emulator's emu::launch.
// A sequence takes plain values (geometry, plans, pointers, booleans), never a context; what the environment says
// arrives as a parameter (kernel_select.hpp), read by each caller where and when it always was -- and the callers
// differ, on purpose left so: the library reads PICSONG_DWT_INV97 once per process for the synthesis levels
// (lean97_levels) but per call, with PICSONG_RGB_NOFUSE, for the RGB tail (rgb_tail_switch, picsong_hip.hip); emu_driver.cpp reads it
// at every call (emu_lean97: the tests flip it); the frame-decode drivers pass a constant true; and emu_fast_div
// re-derives per (qs, wl) what a context stores at its creation.
#pragma once
#include "kernel_select.hpp"

namespace picsong {

// A workspace of the frame pipeline.  The context keeps two: a single frame's, and a batch's with every array n times
// as long, frame after frame; the drivers fill one with pointers into their own arrays.
struct Workspace {
    void *coef;               // T[P + extra]: the transform's work buffer
    int32_t *staging;         // int32[P] (the encoders' 16-bit staging lives in it too)
    int32_t *sizes;           // int32[nCB]
    int32_t *offsets;         // int32[nCB]
    int32_t *total;           // 1
    uint32_t *plane_scratch;  // the coders' bit-planes below the 8 held in registers, 8 KB per wave
    int32_t *coef_i;          // int32[P]: decoded coefficients
};

// ---- element-wise kernels: n4 groups of four samples (level_shift_inv: n samples), `off` the level shift
template <class Go>
int level_shift_fwd(const Go &go, bool lossy, const uint8_t *in, void *out, size_t n4, int off)
{
    const dim3 grid(elementwise_blocks(n4, 4096));
    return lossy ? go(level_shift_fwd_kernel<float>, grid, 256u, in, (float *)out, n4, off)
                 : go(level_shift_fwd_kernel<int32_t>, grid, 256u, in, (int32_t *)out, n4, off);
}
template <class Go>
int level_shift_inv(const Go &go, bool lossy, void *data, size_t n, int off)
{
    const dim3 grid(elementwise_blocks(n));
    return lossy ? go(level_shift_inv_f32_kernel, grid, 256u, (float *)data, n, (float)off)
                 : go(level_shift_inv_i32_kernel, grid, 256u, (int32_t *)data, n, off);
}
// samples of a synthesis that did not write its pixels itself: level shift + clamp
template <class Go>
int clamp_pixels(const Go &go, bool lossy, const void *img, uint8_t *out, size_t n4, int off)
{
    const dim3 grid(elementwise_blocks(n4));
    return lossy ? go(clamp_to_u8_f32_kernel, grid, 256u, (const float *)img, out, n4, (float)off)
                 : go(clamp_to_u8_i32_kernel, grid, 256u, (const int32_t *)img, out, n4, off);
}
// ---- deep contexts: uint16 samples (n4 groups of four; level_shift_inv16: n samples in place), px_max = 2^(bit depth) - 1
template <class Go>
int level_shift_fwd16(const Go &go, bool lossy, const uint16_t *in, void *out, size_t n4, int off)
{
    const dim3 grid(elementwise_blocks(n4, 4096));
    const int wide = (((uintptr_t)in) & 7u) == 0 ? 1 : 0;
    return lossy ? go(level_shift_fwd_u16_kernel<float>, grid, 256u, in, (float *)out, n4, off, wide)
                 : go(level_shift_fwd_u16_kernel<int32_t>, grid, 256u, in, (int32_t *)out, n4, off, wide);
}
template <class Go>
int level_shift_inv16(const Go &go, bool lossy, void *data, size_t n, int off, int px_max)
{
    const dim3 grid(elementwise_blocks(n));
    return lossy ? go(level_shift_inv16_f32_kernel, grid, 256u, (float *)data, n, off, px_max)
                 : go(level_shift_inv16_i32_kernel, grid, 256u, (int32_t *)data, n, off, px_max);
}
template <class Go>
int clamp_pixels16(const Go &go, bool lossy, const void *img, uint16_t *out, size_t n4, int off, int px_max)
{
    const dim3 grid(elementwise_blocks(n4));
    const int wide = (((uintptr_t)out) & 7u) == 0 ? 1 : 0;
    return lossy ? go(clamp_to_u16_f32_kernel, grid, 256u, (const float *)img, out, n4, off, px_max, wide)
                 : go(clamp_to_u16_i32_kernel, grid, 256u, (const int32_t *)img, out, n4, off, px_max, wide);
}
template <class Go>
int rgb_forward(const Go &go, bool lossy, const uint8_t *r, const uint8_t *g, const uint8_t *b, void *c0, void *c1, void *c2,
                size_t n4, int off)
{
    const dim3 grid(elementwise_blocks(n4));
    return lossy ? go(rgb_forward_kernel<float>, grid, 256u, r, g, b, (float *)c0, (float *)c1, (float *)c2, n4, off)
                 : go(rgb_forward_kernel<int32_t>, grid, 256u, r, g, b, (int32_t *)c0, (int32_t *)c1, (int32_t *)c2, n4, off);
}
template <class Go>
int rgb_inverse(const Go &go, bool lossy, const void *c0, const void *c1, const void *c2, uint8_t *r, uint8_t *g, uint8_t *b,
                size_t n4, int off)
{
    const dim3 grid(elementwise_blocks(n4));
    return lossy ? go(rgb_inverse_kernel<float>, grid, 256u, (const float *)c0, (const float *)c1, (const float *)c2, r, g, b, n4, off)
                 : go(rgb_inverse_kernel<int32_t>, grid, 256u, (const int32_t *)c0, (const int32_t *)c1, (const int32_t *)c2, r, g, b, n4, off);
}
// ---- deep RGB contexts: the colour transforms on uint16 samples, ONE launch over the n frames of a call (grid.y = frame):
// frame f's sample planes smp_z bytes after r / g / b, its T planes cmp_z bytes after c0 / c1 / c2.  The 8-byte accesses
// where every sample plane of every frame is 8-byte aligned, 2-byte ones otherwise: the same values.
inline Rgb16Args rgb16_args(const void *c0, const void *c1, const void *c2, const void *r, const void *g, const void *b, size_t n4,
                            int off, int px_max, unsigned n, unsigned long long cmp_z, unsigned long long smp_z)
{
    Rgb16Args a;
    memset(&a, 0, sizeof a);
    a.c0 = c0; a.c1 = c1; a.c2 = c2; a.r = r; a.g = g; a.b = b;
    a.cmp_z = n > 1 ? cmp_z : 0; a.smp_z = n > 1 ? smp_z : 0;
    a.n4 = n4; a.off = off; a.mx = px_max;
    a.wide = (((((uintptr_t)r) | ((uintptr_t)g) | ((uintptr_t)b)) & 7u) == 0 && (a.smp_z & 7u) == 0) ? 1 : 0;
    return a;
}
inline dim3 rgb16_grid(size_t n4, unsigned n)
{
    // (a frame's workgroups as ever, grid-stride beyond the cap the n frames share)
    return dim3(elementwise_blocks(n4, 8192u / n > 0 ? 8192u / n : 1u), n);
}
template <class Go>
int rgb_forward16(const Go &go, bool lossy, const uint16_t *r, const uint16_t *g, const uint16_t *b, void *c0, void *c1, void *c2,
                  size_t n4, int off, unsigned n = 1, unsigned long long smp_z = 0, unsigned long long cmp_z = 0)
{
    const Rgb16Args a = rgb16_args(c0, c1, c2, r, g, b, n4, off, 0, n, cmp_z, smp_z);
    return lossy ? go(rgb_forward16_kernel<float>, rgb16_grid(n4, n), 256u, a) : go(rgb_forward16_kernel<int32_t>, rgb16_grid(n4, n), 256u, a);
}
template <class Go>
int rgb_inverse16(const Go &go, bool lossy, const void *c0, const void *c1, const void *c2, uint16_t *r, uint16_t *g, uint16_t *b,
                  size_t n4, int off, int px_max, unsigned n = 1, unsigned long long cmp_z = 0, unsigned long long smp_z = 0)
{
    const Rgb16Args a = rgb16_args(c0, c1, c2, r, g, b, n4, off, px_max, n, cmp_z, smp_z);
    return lossy ? go(rgb_inverse16_kernel<float>, rgb16_grid(n4, n), 256u, a) : go(rgb_inverse16_kernel<int32_t>, rgb16_grid(n4, n), 256u, a);
}

// ---- forward transform.  Levels [from, end) of a plan, one launch each; `frames` = grid.z of a batched call.
template <class Go>
int launch_fwd_levels(const Go &go, bool lossy, const std::vector<FwdLaunch> &plan, size_t from, unsigned frames = 1)
{
    for (size_t l = from; l < plan.size(); l++) {
        const FwdLaunch &f = plan[l];
        if (int rc = go(select_fwd(lossy, f), dim3(f.gx, f.gy, frames), 256u, f.a)) return rc;
    }
    return 0;
}
// A forward plan, levels 0 and 1 in one launch where plan_dwt_fwd2 allows it (LL1 stays in registers); *fused01 says so
template <class Go>
int launch_fwd_plan(const Go &go, bool lossy, const std::vector<FwdLaunch> &plan, unsigned frames = 1, bool *fused01 = nullptr)
{
    Fwd2Launch f2;
    const int nb = f2_pairs_batched(plan, lossy, frames);
    const bool fused = plan_dwt_fwd2(plan, f2, true, lossy, nb);
    if (fused01) *fused01 = fused;
    if (fused)
        if (int rc = go(select_fwd2(lossy, f2.a.l0.c16 != 0, false, nb), dim3(f2.gx, f2.gy, frames), 256u, f2.a)) return rc;
    return launch_fwd_levels(go, lossy, plan, fused ? 2 : 0, frames);
}
// a batched forward plan: level 0 reads frame z at + z * src_z0 bytes, every level works in frame z's buffer of coef_z bytes
inline void plan_frame_strides(std::vector<FwdLaunch> &plan, unsigned long long src_z0, unsigned long long coef_z)
{
    for (size_t l = 0; l < plan.size(); l++) {
        plan[l].a.src_z = l == 0 ? src_z0 : coef_z;
        plan[l].a.dst_z = coef_z;
    }
}
// The forward transform of n deep frames (picsong_encode_frames16, picsong_dwt_forward_u16): uint16 samples at `frames`,
// frame_stride bytes apart, frame f's coefficients in its buffer of coef_z bytes at coef.  Level 0 reads the samples
// itself (plan_dwt_forward_u16), or -- nofuse (PICSONG_DEEP_NOFUSE=1: the caller reads it) -- a level shift a frame into
// `shifted` (P samples of T a frame, 16-byte aligned) and the T-input plan.  *in_kernel says which ran.
template <class Go>
int deep_forward(const Go &go, bool lossy, bool nofuse, const uint16_t *frames, size_t frame_stride, unsigned n, void *coef, void *shifted,
                 int aw, int ah, int wl, float qs, int off, unsigned long long coef_z, bool *in_kernel = nullptr)
{
    const size_t P = (size_t)aw * (size_t)ah;
    if (n <= 1) frame_stride = 0;
    if (in_kernel) *in_kernel = !nofuse;
    if (!nofuse) {
        std::vector<FwdLaunch> plan = plan_dwt_forward_u16(frames, frame_stride, n, coef, aw, ah, wl, qs, off);
        plan_frame_strides(plan, frame_stride, coef_z);
        return launch_fwd_levels(go, lossy, plan, 0, n);
    }
    for (unsigned f = 0; f < n; f++)
        if (int rc = level_shift_fwd16(go, lossy, (const uint16_t *)((const char *)frames + (size_t)f * frame_stride),
                                       (char *)shifted + (size_t)f * P * 4, P / 4, off)) return rc;
    std::vector<FwdLaunch> plan = plan_dwt_forward(shifted, false, coef, aw, ah, wl, qs, false);
    plan_frame_strides(plan, (unsigned long long)P * 4ull, coef_z);
    return launch_fwd_levels(go, lossy, plan, 0, n);
}

// The forward transform of n deep RGB frames (picsong_encode_rgb_frames16): uint16 planes at r / g / b, frame f's
// frame_stride bytes behind; plane z = component z % 3 of frame z / 3, its coefficients in its buffer of coef_z bytes at
// coef; one launch a level (grid.z = 3 n).  Level 0 reads the three sample planes of a frame and applies the colour
// transform itself (plan_dwt_forward_rgb16), so no component plane is ever written; or -- nofuse (PICSONG_DEEP_NOFUSE=1:
// the caller reads it) -- the colour transform of the n frames as ONE launch (rgb_forward16) into `planes` (3 n planes of
// P samples of T, 16-byte aligned), then the T-input plan.  Always the 32-bit coefficient form.  *in_kernel says which ran.
template <class Go>
int deep_rgb_forward(const Go &go, bool lossy, bool nofuse, const uint16_t *r, const uint16_t *g, const uint16_t *b, size_t frame_stride,
                     unsigned n, void *coef, void *planes, int aw, int ah, int wl, float qs, int off, unsigned long long coef_z,
                     bool *in_kernel = nullptr)
{
    const size_t P = (size_t)aw * (size_t)ah;
    if (n <= 1) frame_stride = 0;
    if (in_kernel) *in_kernel = !nofuse;
    if (!nofuse) {
        std::vector<FwdLaunch> plan = plan_dwt_forward_rgb16(r, g, b, frame_stride, n, coef, aw, ah, wl, qs, off);
        plan_frame_strides(plan, frame_stride, coef_z);      // level 0: every component of a frame reads its three planes
        return launch_fwd_levels(go, lossy, plan, 0, 3u * n);
    }
    char *q = (char *)planes;
    if (int rc = rgb_forward16(go, lossy, r, g, b, q, q + P * 4, q + 2 * P * 4, P / 4, off, n, frame_stride, 3ull * P * 4ull)) return rc;
    std::vector<FwdLaunch> plan = plan_dwt_forward(planes, false, coef, aw, ah, wl, qs, false);
    plan_frame_strides(plan, (unsigned long long)P * 4ull, coef_z);
    return launch_fwd_levels(go, lossy, plan, 0, 3u * n);
}

// An RGB frame's colour transform (level shift fused) and the forward transform of its three components, component k's
// coefficients coef_z bytes after component k - 1's.  plan_of(src, u8in) makes the caller's plan: plan_dwt_forward with
// its c16 choice (head_c16: the fused head is the frame paths' 16-bit one and wants such a plan) or the rate calls'
// plan_dwt_forward_unit (the 32-bit float head, select_fwd2_rgb_f32).
// fuse (the caller's switches: planes 16-byte aligned, no PICSONG_RGB_NOFUSE, its c16 choice): the colour transform in
// the head's load stage -- the head reads the three u8 planes and delivers component blockIdx.z % 3, no component plane is
// ever written (the separate transform kernel reads 100 MB and writes 400 MB of them per 8K frame, and level 0 reads
// them back).  Else, or where plan_dwt_fwd2 refuses: the colour transform into `planes` (three of P samples a frame),
// then the levels of all planes per launch.  *c16: the coefficient form delivered; *fused: the first form ran.
// n frames (picsong_encode_rgb_frames): frame f's planes frame_stride bytes after frame f - 1's, its component k's
// coefficients in plane 3 f + k; every launch but the separate colour transform's (one a frame) covers the 3 n planes.
template <class Go, class PlanOf>
int rgb_forward_transform(const Go &go, bool lossy, bool fuse, PlanOf plan_of, bool head_c16, const uint8_t *r, const uint8_t *g,
                          const uint8_t *b, void *planes, size_t P, int off, unsigned long long coef_z, bool *c16 = nullptr,
                          bool *fused = nullptr, unsigned n = 1, unsigned long long frame_stride = 0)
{
    if (fused) *fused = false;
    if (n <= 1) frame_stride = 0;
    if (fuse) {
        std::vector<FwdLaunch> plan = plan_of(r, true);
        plan_frame_strides(plan, frame_stride, coef_z);      // level 0: every component of a frame reads its three planes
        plan[0].a.src_g = g; plan[0].a.src_b = b;
        Fwd2Launch f2;
        if (plan_is_c16(plan) == head_c16 && plan_dwt_fwd2(plan, f2, true, lossy, kF2PairsRgb)) {
            // (RCT on the integer head, ICT on the 9/7 ones)
            if (int rc = go(head_c16 ? select_fwd2(lossy, true, true) : select_fwd2_rgb_f32(), dim3(f2.gx, f2.gy, 3u * n), 256u, f2.a)) return rc;
            if (c16) *c16 = head_c16;
            if (fused) *fused = true;
            return launch_fwd_levels(go, lossy, plan, 2, 3u * n);
        }
    }
    char *p = (char *)planes;
    for (unsigned f = 0; f < n; f++) {
        char *q = p + (size_t)f * 3 * P * 4;
        const size_t at = (size_t)f * (size_t)frame_stride;
        if (int rc = rgb_forward(go, lossy, r + at, g + at, b + at, q, q + P * 4, q + 2 * P * 4, P / 4, off)) return rc;
    }
    std::vector<FwdLaunch> plan = plan_of(planes, false);
    if (c16) *c16 = plan_is_c16(plan);
    plan_frame_strides(plan, (unsigned long long)P * 4ull, coef_z);
    return launch_fwd_levels(go, lossy, plan, 0, 3u * n);
}

// ---- synthesis.  The first n levels of a plan (plan_inverse_frames), one launch each
template <class Go>
int launch_inv_levels(const Go &go, bool lossy, bool lean97, const std::vector<InvLaunch> &plan, size_t n, unsigned frames)
{
    for (size_t l = 0; l < n; l++) {
        const InvLaunch &f = plan[l];
        if (int rc = go(select_inv(lossy, lean97, f), dim3(f.gx, f.gy, frames), 256u, f.a)) return rc;
    }
    return 0;
}
// A synthesis plan; 16-bit coefficients in, pixels out: levels 1 and 0 as one launch (dwt_inv2_kernel), LL0 in
// registers, where plan_dwt_inv2 allows it -- *fused10 says so
template <class Go>
int run_inverse(const Go &go, bool lossy, bool lean97, const std::vector<InvLaunch> &plan, unsigned frames = 1, bool *fused10 = nullptr)
{
    Inv2Launch f2;
    const bool fused = plan_dwt_inv2(plan, f2, lossy);
    if (fused10) *fused10 = fused;
    if (int rc = launch_inv_levels(go, lossy, lean97, plan, fused ? plan.size() - 2 : plan.size(), frames)) return rc;
    return fused ? go(select_inv2(lossy, f2.a.l0.one_div != 0), dim3(f2.gx, f2.gy, frames), 256u, f2.a) : 0;
}
// An RGB frame's synthesis with 16-bit coefficients (plan_inverse_frames over three components, planes_out): the levels
// above the finest, then the finest level of the three components and the inverse colour transform as ONE launch
// (select_inv_rgb).  5/3: the 32-bit planes are never written (dwt_inv_rgb_kernel).  9/7, the lean kernel's domain: the
// three components as the three waves of a workgroup, a row pair exchanged through LDS, the inverse ICT at the stores
// (dwt_inv97_rgb_kernel).  inv_rgb_tail_ok: may the plan take that form?  (9/7: the caller's lean97 switch permitting)
inline bool inv_rgb_tail_ok(const std::vector<InvLaunch> &plan, bool lossy)
{
    return plan_inv_is_c16(plan) && plan.size() >= 2 && plan.back().vec && (!lossy || plan.back().fast);
}
// n frames (picsong_decode_rgb_frames; the plan over 3 n planes): grid.z = 3 n above the finest level, = frame in the tail,
// frame f's pixel planes frame_stride bytes after frame f - 1's
template <class Go>
int run_inverse_rgb(const Go &go, bool lossy, bool lean97, const std::vector<InvLaunch> &plan, int off, uint8_t *r, uint8_t *g, uint8_t *b,
                    unsigned n = 1, unsigned long long frame_stride = 0)
{
    if (int rc = launch_inv_levels(go, lossy, lean97, plan, plan.size() - 1, 3u * n)) return rc;
    DwtInvArgs fa = plan.back().a;
    fa.off = off;
    fa.u8_z = n > 1 ? frame_stride : 0;
    const InvRgbLaunch l = select_inv_rgb(lossy, plan.back());
    return go(l.kernel, dim3(l.gx, l.gy, n), l.threads, fa, r, g, b);
}

// ---- the windowed synthesis (window_kernels.hpp) of `frames` frames, grid.z = frame: frame z's coefficients at coef_i +
// z * coef_z bytes, its scratch (T[P + extra]) at work + z * work_z bytes.  u8 != nullptr: level r writes frame z's
// window at u8 + z * u8_z, row stride pitch; else level r's samples stay at frame z's `work` (compact, row stride w).
// px_max > 0 (a deep context): the window holds uint16 samples clamped to px_max; pitch and u8_z stay in bytes.
template <class Go>
int run_window(const Go &go, bool lossy, const WindowPlan &w, const int32_t *coef_i, void *work, size_t P, int aw, int ah, float qs,
               int off, unsigned frames, unsigned long long coef_z, unsigned long long work_z, uint8_t *u8, size_t pitch,
               unsigned long long u8_z, int px_max = 0)
{
    for (WinLaunch &f : plan_window_synthesis(w, coef_i, work, P, aw, ah, qs, u8, pitch, off, px_max)) {
        f.a.mallat_z = coef_z; f.a.ll_z = work_z; f.a.dst_z = work_z; f.a.u8_z = u8_z;
        f.grid.z = frames;
        if (int rc = go(select_window_out(lossy, f.out), f.grid, 256u, f.a)) return rc;
    }
    return 0;
}

// ---- stream intake: the codeblock lengths of n streams `stride` shorts apart into w.sizes, their scan into w.offsets
// and w.total -- `direct`, one launch, for a decoder that reads the streams itself; else the codewords unpacked into
// w.staging (frame f's at + f * P words) as well (-k > 0 through the staging, -cp 3, PICSONG_DEC_STAGING)
template <class Go>
int stream_intake(const Go &go, const uint16_t *streams, unsigned n, size_t stride, bool direct, int ncb, size_t P,
                  const Workspace &w, int *flag)
{
    if (direct) return go(scan_stream_kernel, dim3(n), scan_threads(ncb), streams, ncb, w.sizes, w.offsets, w.total, flag, stride);
    if (int rc = go(read_sizes_kernel, dim3((unsigned)((ncb + 255) / 256), n), 256u, streams, ncb, w.sizes, flag, stride)) return rc;
    if (int rc = go(scan_sizes_kernel, dim3(n), scan_threads(ncb), w.sizes, ncb, w.offsets, w.total)) return rc;
    return go(unpack_kernel, dim3((unsigned)ncb, n), 256u, streams, w.sizes, w.offsets, ncb, w.staging, stride, P);
}

// ---- the coders.  kLaunchRefused: no kernel exists for what the caller asks (nothing launched)
constexpr int kLaunchRefused = -1000;
// The decoder launch of every path: `waves` waves over w's sizes, staging and plane scratch, coefficients into w.coef_i.
// streams != nullptr (k = 0 or -k > 0, -cp 2): the codewords come from the packed streams, `stride` shorts apart and at
// most cw16_max long, at w.offsets (stream_intake's scan); w.staging is then not read
// c16 (with streams): the coefficients leave as int16 Mallat arrays (bpc_decode_kernel's C16 form)
// compact: the tables of the launch take the COMPACT copies (-k > 0, bulk_compact)
// a.drop > 0 (picsong_ctx_set_decode_drop; k = 0, -cp 2): the reduced-quality kernels -- same grid, same arguments
template <class Go>
int launch_decoder(const Go &go, BpcArgs &a, bool cp3, unsigned waves, bool compact, const Workspace &w, const uint16_t *streams,
                   size_t stride, uint32_t cw16_max, bool c16)
{
    const BpcLaunch l = select_decoder(cp3, a.k > 0.0f, compact, streams != nullptr, c16, waves, a.drop > 0);
    if (!l.kernel) return kLaunchRefused;
    a.coeffs_out = w.coef_i; a.staging = w.staging; a.sizes = w.sizes; a.plane_scratch = w.plane_scratch;
    if (streams) { a.cw16 = streams; a.cw16_offsets = w.offsets; a.cw16_total = w.total; a.cw16_stride = stride; a.cw16_max = cw16_max; }
    return go(l.kernel, dim3(l.wgs), l.threads, a);
}
// The encoder launch of every path: `waves` waves (a codeblock pair each), the caller's `a` complete but for the kernel's choice
template <class Go>
int launch_encoder(const Go &go, const BpcArgs &a, bool cp3, bool compact_pipelined, unsigned waves)
{
    const BpcLaunch l = select_encoder(cp3, a.k > 0.0f, a.k > 0.0f && compact_pipelined, waves);
    return go(l.kernel, dim3(l.wgs), l.threads, a);
}
// the stage API's int32 array from the encoders' 16-bit staging: words 0 .. len - 1 of codeblocks [cb_base, cb_base + n)
template <class Go>
int widen_staging(const Go &go, const uint16_t *staging16, const int32_t *sizes, int cb_base, int n, int32_t *staging)
{
    return go(widen_staging_kernel, dim3((unsigned)n), 256u, staging16, sizes, cb_base, staging);
}

// ---- THE decode sequence of every frame call -- grey or RGB, 1 or n frames, whole, at 1/2^reduce or a window: the
// intake of the streams, the decoder over the call's codeblocks, the synthesis, its tail; every stage ONE launch over the
// call's planes.  Grey: a plane a frame.  Colour: 3 n planes, plane z = component z % 3 of frame z / 3, table z % 3.
// n = 1 sets BpcArgs::frames = 1 (colour: 3), the single-frame launch.  What a context holds for it:
struct DecodeCtx {
    int aw, ah, wl, ncb;
    bool lossy; float qs; bool fast_div; int off;
    size_t P, extra;
    bool rgb = false;         // colour: `a` holds the three tables on one coder grid (bpc_args_rgb), w 3 n planes
    bool cp3 = false;         // -cp 3 (picsong_decode_frame alone, through the staging)
    bool direct;              // the decoder reads the streams itself (else: through the staging)
    bool compact;             // -k > 0: the launch takes the COMPACT table copies
    uint32_t max_stream;      // a worst-case stream's shorts
    int *flag;                // the intake's damage flag
    int px_max = 0;           // > 0: a deep context -- the grey calls' `out` holds uint16 samples, clamped to [0, px_max]
};
// what a call took, for those who ask (the drivers' return bits)
struct DecodeReport {
    bool pixels;              // grey: the finest level wrote the pixels itself
    bool c16;                 // the coefficients travelled as int16
    bool fused10;             // levels reduce + 1 and reduce ran as one launch (run_inverse)
    bool rgb_tail;            // colour: the fused tail ran (run_inverse_rgb)
    bool vec;                 // colour window: the epilogue's vector form ran
};
// The head: the intake, the call's rectangle (every codeblock, the reduced corner, or win's table), the synthesis plan
// (none for a window: the cone's synthesis reads 32-bit coefficients) -- planned ahead of the decoder, for it says
// whether this call's coefficients can travel as int16 -- and the decoder's one grid.  pixels: the grey destination
// (frames pix_stride bytes apart) the finest level may write itself.
template <class Go>
int decode_head(const Go &go, const DecodeCtx &c, BpcArgs &a, const Workspace &w, unsigned n, const uint16_t *streams, size_t stream_stride,
                int reduce, const WindowPlan *win, bool want_c16, uint8_t *pixels, size_t pix_stride, std::vector<InvLaunch> &plan,
                DecodeReport &rep)
{
    const unsigned np = c.rgb ? 3u * n : n;
    rep = DecodeReport();
    if (int rc = stream_intake(go, streams, np, stream_stride, c.direct, c.ncb, c.P, w, c.flag)) return rc;
    int wpf = (c.ncb + 1) / 2;
    if (win) {
        wpf = window_bpc_table(a, *win);
    } else if (reduce > 0) {
        const ReducedRect q = reduced_rect(c.aw, c.ah, reduce);
        a.ncx_r = q.ncx_r; a.ncb_r = q.ncx_r * q.ncy_r;
        wpf = reduced_waves(q);
    }
    a.cb_base = 0; a.nCB = c.ncb;
    a.frames = (int)np; a.waves_per_frame = c.rgb ? rgb_component_waves(a.k > 0.0f, wpf) : wpf;
    if (!win)
        plan = plan_inverse_frames(w.coef_i, w.coef, pixels, &rep.pixels, np, pix_stride, want_c16 && c.direct, c.rgb, reduce, c.aw, c.ah,
                                   c.wl, c.qs, c.fast_div, c.off, c.P, c.extra, c.px_max);
    rep.c16 = plan_inv_is_c16(plan);
    a.coef_z = (unsigned long long)c.P * (rep.c16 ? 2ull : 4ull);
    return launch_decoder(go, a, c.cp3, np * (unsigned)a.waves_per_frame, c.compact, w, c.direct ? streams : nullptr, stream_stride,
                          c.max_stream, rep.c16);
}
// The grey calls (picsong_decode_frame, picsong_decode_frames, their _reduced and _window forms): frame f's pixels of
// level `reduce`, row stride aw >> reduce, at out + f * frame_stride -- written by the finest level where its vector
// kernel applies, else by a clamp a frame; win: frame f's window of that level, row stride pitch.
template <class Go>
int decode_frames(const Go &go, const DecodeCtx &c, BpcArgs a, const Workspace &w, unsigned n, const uint16_t *streams, size_t stream_stride,
                  int reduce, const WindowPlan *win, bool want_c16, bool lean97, uint8_t *out, size_t frame_stride, size_t pitch,
                  DecodeReport *report = nullptr)
{
    DecodeReport mine, &rep = report ? *report : mine;
    std::vector<InvLaunch> plan;
    if (n <= 1) frame_stride = 0;
    if (int rc = decode_head(go, c, a, w, n, streams, stream_stride, reduce, win, want_c16, out, frame_stride, plan, rep)) return rc;
    const size_t z = (c.P + c.extra) * 4, n4 = (size_t)(c.aw >> reduce) * (size_t)(c.ah >> reduce) / 4;
    // (a deep context, px_max > 0: level r stores uint16 samples, pitch and frame_stride in bytes)
    if (win) return run_window(go, c.lossy, *win, w.coef_i, w.coef, c.P, c.aw, c.ah, c.qs, c.off, n, (unsigned long long)c.P * 4ull, z, out, pitch, frame_stride, c.px_max);
    if (int rc = run_inverse(go, c.lossy, lean97, plan, n, &rep.fused10)) return rc;
    // (level `reduce`'s samples of frame f: c.extra elements into its work buffer when reduce = 0)
    for (unsigned f = 0; f < n && !rep.pixels; f++) {
        if (c.px_max > 0) {
            if (int rc = clamp_pixels16(go, c.lossy, (const char *)plan.back().a.dst + f * z, (uint16_t *)(out + f * frame_stride), n4, c.off, c.px_max)) return rc;
        } else if (int rc = clamp_pixels(go, c.lossy, (const char *)plan.back().a.dst + f * z, out + f * frame_stride, n4, c.off)) return rc;
    }
    return 0;
}
// The colour calls (picsong_decode_rgb_frame, picsong_decode_rgb_frames, their _reduced and _window forms, the image
// calls over them), frames frame_stride bytes apart.
// win == nullptr: frame f's planes of (aw >> reduce) x (ah >> reduce) bytes at d0 / d1 / d2 + f * frame_stride.  The inverse
// colour transform in the finest level's launch (run_inverse_rgb, grid.z = frame) where the plan has that form and every
// frame's planes are 4-byte aligned (fuse_tail: the caller's switches permitting), else on its own, one launch a frame.
// win: run_window with frames = 3 n, level r's samples left compact in the planes' work buffers, and the epilogue
// (window_rgb_image_kernel, grid.z = frame) that stores them in `layout`: d0 .. d2 frame 0's R, G, B planes
// (kLayoutPlanar3), or d0 its interleaved pixels; rows `pitch` bytes apart.  One frame into planar planes: window_rgb_kernel.
// A deep RGB context (px_max > 0): uint16 samples, `layout` one of the three 16-bit ones, pitch and frame_stride in bytes --
// the reduced planes through rgb_inverse16 over (aw >> reduce) x (ah >> reduce) samples, a window through window_rgb16_image_kernel.
template <class Go>
int decode_rgb_frames(const Go &go, const DecodeCtx &c, BpcArgs a, const Workspace &w, unsigned n, const uint16_t *streams,
                      size_t stream_stride, int reduce, const WindowPlan *win, bool want_c16, bool lean97, bool fuse_tail, int layout,
                      uint8_t *d0, uint8_t *d1, uint8_t *d2, size_t pitch, size_t frame_stride, DecodeReport *report = nullptr)
{
    DecodeReport mine, &rep = report ? *report : mine;
    std::vector<InvLaunch> plan;
    if (n <= 1) frame_stride = 0;
    if (int rc = decode_head(go, c, a, w, n, streams, stream_stride, reduce, win, want_c16, nullptr, 0, plan, rep)) return rc;
    const size_t z = (c.P + c.extra) * 4, n4 = (size_t)(c.aw >> reduce) * (size_t)(c.ah >> reduce) / 4;
    if (win) {
        if (int rc = run_window(go, c.lossy, *win, w.coef_i, w.coef, c.P, c.aw, c.ah, c.qs, c.off, 3u * n, (unsigned long long)c.P * 4ull, z,
                                nullptr, 0, 0)) return rc;
        const IRect &o = win->R[win->r];
        if (c.px_max > 0) {
            // a deep RGB context: uint16 samples in kLayoutPlanar3_16, kLayoutRgb48 or kLayoutRgba64, one launch whatever n
            const WinRgb16Args ra = window_rgb16_args(layout, w.coef, z, o.x1 - o.x0, o.y1 - o.y0, d0, d1, d2, pitch, frame_stride, n, c.off, c.px_max);
            const WinRgb16Launch l = select_window_rgb16(c.lossy, layout, ra, n);
            if (!l.kernel) return kLaunchRefused;
            rep.vec = l.vec;
            return go(l.kernel, l.grid, 256u, ra);
        }
        // (one frame into planar planes keeps the per-pixel epilogue: measured against the n-frame one, profiles/NOTES.md)
        if (n == 1 && layout == kLayoutPlanar3) {
            const dim3 grid((unsigned)((o.x1 - o.x0 + 255) / 256), (unsigned)(o.y1 - o.y0));
            return c.lossy ? go(window_rgb_kernel<float>, grid, 256u, (const float *)w.coef, (unsigned long long)z, o.x1 - o.x0, o.y1 - o.y0, d0, d1, d2, (unsigned long long)pitch, c.off)
                           : go(window_rgb_kernel<int>, grid, 256u, (const int *)w.coef, (unsigned long long)z, o.x1 - o.x0, o.y1 - o.y0, d0, d1, d2, (unsigned long long)pitch, c.off);
        }
        const WinRgbArgs ra = window_rgb_args(layout, w.coef, z, o.x1 - o.x0, o.y1 - o.y0, d0, d1, d2, pitch, frame_stride, n, c.off);
        const WinRgbLaunch l = select_window_rgb(c.lossy, layout, ra, n);
        rep.vec = l.vec;
        return go(l.kernel, l.grid, 256u, ra);
    }
    if (c.px_max > 0) {
        // a deep RGB context (picsong_decode_rgb_frames16): d0 .. d2 hold uint16 samples.  The synthesis writes the 3 n T
        // planes (plan_inverse_frames' deep plan, no pixel destination), then ONE inverse-transform launch over the n frames
        if (int rc = run_inverse(go, c.lossy, lean97, plan, 3u * n, &rep.fused10)) return rc;
        const char *img = (const char *)plan.back().a.dst;
        return rgb_inverse16(go, c.lossy, img, img + z, img + 2 * z, (uint16_t *)d0, (uint16_t *)d1, (uint16_t *)d2, n4, c.off, c.px_max, n,
                             3ull * z, frame_stride);
    }
    const bool px_aligned = ((((uintptr_t)d0) | ((uintptr_t)d1) | ((uintptr_t)d2) | frame_stride) & 3u) == 0;
    rep.rgb_tail = fuse_tail && px_aligned && inv_rgb_tail_ok(plan, c.lossy);
    if (rep.rgb_tail) return run_inverse_rgb(go, c.lossy, lean97, plan, c.off, d0, d1, d2, n, frame_stride);
    if (int rc = run_inverse(go, c.lossy, lean97, plan, 3u * n, &rep.fused10)) return rc;
    for (unsigned f = 0; f < n; f++) {
        // (level `reduce`'s samples of frame f's components: c.extra elements into their work buffers when reduce = 0)
        const char *img = (const char *)plan.back().a.dst + (size_t)(3 * f) * z;
        const size_t at = (size_t)f * frame_stride;
        if (int rc = rgb_inverse(go, c.lossy, img, img + z, img + 2 * z, d0 + at, d1 + at, d2 + at, n4, c.off)) return rc;
    }
    return 0;
}
// The colour sequence's two forms under the names and signatures the n-frame RGB proxy calls introduced them with, for
// callers written against those (a context they filled says nothing of colour or -cp 3: set here).  *fused: the fused tail
// ran; *vec: the epilogue's vector form ran.
using RgbProxyCtx = DecodeCtx;
template <class Go>
int decode_rgb_frames_reduced(const Go &go, RgbProxyCtx c, const BpcArgs &a, const Workspace &w, unsigned n, const uint16_t *streams,
                              size_t stream_stride, int reduce, bool want_c16, bool lean97, bool fuse_tail, uint8_t *r, uint8_t *g,
                              uint8_t *b, unsigned long long frame_stride, bool *fused = nullptr)
{
    DecodeReport rep = DecodeReport();
    c.rgb = true; c.cp3 = false;
    const int rc = decode_rgb_frames(go, c, a, w, n, streams, stream_stride, reduce, nullptr, want_c16, lean97, fuse_tail, kLayoutPlanar3, r, g,
                                     b, 0, (size_t)frame_stride, &rep);
    if (fused) *fused = rep.rgb_tail;
    return rc;
}
template <class Go>
int decode_rgb_frames_window(const Go &go, RgbProxyCtx c, const BpcArgs &a, const Workspace &w, unsigned n, const uint16_t *streams,
                             size_t stream_stride, const WindowPlan &win, int layout, uint8_t *d0, uint8_t *d1, uint8_t *d2, size_t pitch,
                             size_t frame_stride, bool *vec = nullptr)
{
    DecodeReport rep = DecodeReport();
    c.rgb = true; c.cp3 = false;
    const int rc = decode_rgb_frames(go, c, a, w, n, streams, stream_stride, win.r, &win, false, false, false, layout, d0, d1, d2, pitch,
                                     frame_stride, &rep);
    if (vec) *vec = rep.vec;
    return rc;
}

// ---- the pack of n frames' codeblocks, frame after frame in w (sizes, offsets, totals) and in the staging (P words a
// frame): the header argument, the scan of the lengths, the copy into streams `stream_stride` shorts apart.
// W: uint16_t = the encoders' own staging (the frame paths), int32_t = a caller's array (picsong_bitstream_pack)
// h_header != nullptr: the populated header, on the frames `has` and `base` name (HeaderArg, pack_kernels.hpp)
template <typename W, class Go>
int pack_frames(const Go &go, const W *staging, const Workspace &w, int ncb, unsigned n, const uint16_t *h_header, int has,
                uint16_t *streams, size_t P, size_t stream_stride, int base = 0)
{
    HeaderArg h;
    memset(&h, 0, sizeof h);
    if (h_header) { memcpy(h.h, h_header, sizeof h.h); h.has = has; h.base = base; }
    if (int rc = go(scan_sizes_kernel, dim3(n), scan_threads(ncb), w.sizes, ncb, w.offsets, w.total)) return rc;
    return go(pack_kernel<W>, dim3(pack_blocks<W>(ncb), n), 256u, staging, w.sizes, w.offsets, w.total, ncb, h, streams, P, stream_stride);
}

// the pack of n RGB frames' 3 n planes (picsong_encode_rgb_frames): the populated header h_header on the components
// header_mask names (bits 0..2) of the frame f with first_iter + f == 0, where the call holds it; none anywhere else
template <class Go>
int pack_rgb_frames(const Go &go, const uint16_t *staging, const Workspace &w, int ncb, unsigned n, const uint16_t *h_header,
                    int first_iter, int header_mask, uint16_t *streams, size_t P, size_t stream_stride)
{
    const int f0 = -first_iter;
    const bool has0 = f0 >= 0 && f0 < (int)n && (header_mask & 7) != 0;
    return pack_frames(go, staging, w, ncb, 3u * n, has0 ? h_header : nullptr, -(header_mask & 7), streams, P, stream_stride,
                       has0 ? 3 * f0 : 0);
}

// ---- distortion (quality_kernels.hpp): out[0 .. n) = the SSE over the visible w x h samples of n pairs of padded
// arrays, zeroed on the launcher's stream first
template <class Go>
int frames_sse(const Go &go, const uint8_t *a, size_t a_pitch, unsigned long long a_z, const uint8_t *b, size_t b_pitch,
               unsigned long long b_z, int w, int h, int n, unsigned long long *out)
{
    if (int rc = go(sse_zero_kernel, dim3(1), 64u, out, n)) return rc;
    const SseArgs s = sse_args(a, a_pitch, a_z, b, b_pitch, b_z, w, h, n, out);
    return go(select_sse(s).kernel, dim3(select_sse(s).wgs), 256u, s);
}
// ---- structural distortion (ssim_kernel, quality_kernels.hpp): out[0 .. n) = the DSSIM sum (windows * 2^24 - the sum
// of the windows' q: the kernel adds 2^24 - q a window, no conversion on the host) over the visible w x h samples,
// w, h >= 8, of n pairs of padded arrays, zeroed on the launcher's stream first
template <class Go>
int frames_dssim(const Go &go, const uint8_t *a, size_t a_pitch, unsigned long long a_z, const uint8_t *b, size_t b_pitch,
                 unsigned long long b_z, int w, int h, int n, unsigned long long *out)
{
    if (int rc = go(sse_zero_kernel, dim3(1), 64u, out, n)) return rc;
    const SseArgs s = sse_args(a, a_pitch, a_z, b, b_pitch, b_z, w, h, n, out);
    return go(select_ssim(s).kernel, dim3(select_ssim(s).wgs), 256u, s);
}

// ---- pixel layouts (layout_kernels.hpp): n frames of W x H pixels at a pitch into padded planar planes, and back.  The
// arguments have passed layout_refusal.  *vec: the vector form ran
template <class Go>
int ingest_frames(const Go &go, int layout, const void *data, size_t pitch, size_t plane_stride, size_t frame_stride, uint8_t *padded,
                  size_t padded_stride, int n, int W, int H, int AW, int AH, bool *vec = nullptr, int px_max = 0)
{
    const LayoutArgs a = layout_args(layout, data, pitch, plane_stride, frame_stride, padded, padded_stride, n, W, H, AW, AH, px_max);
    LayoutLaunch l = select_ingest(layout, a);
    l.grid.z = (unsigned)n;
    if (vec) *vec = l.vec;
    return go(l.kernel, l.grid, 256u, a);
}
template <class Go>
int emit_frames(const Go &go, int layout, const uint8_t *padded, size_t padded_stride, void *data, size_t pitch, size_t plane_stride,
                size_t frame_stride, int n, int W, int H, int AW, int AH, bool *vec = nullptr, int px_max = 0)
{
    const LayoutArgs a = layout_args(layout, data, pitch, plane_stride, frame_stride, padded, padded_stride, n, W, H, AW, AH, px_max);
    LayoutLaunch l = select_emit(layout, a);
    l.grid.z = (unsigned)n;
    if (vec) *vec = l.vec;
    return go(l.kernel, l.grid, 256u, a);
}

// picsong_decode_rgb_images_reduced where reduced_emit_ok: decode_rgb_frames_reduced into `lay` -- 3 n planes of paw x pah
// bytes, R, G, B back to back per frame, 16-byte aligned, so the fused tail runs where the plan has it -- then ONE emit of
// the visible rw x rh pixels of the n frames into the caller's layout
template <class Go>
int decode_rgb_images_reduced(const Go &go, const DecodeCtx &c, const BpcArgs &a, const Workspace &w, unsigned n, const uint16_t *streams,
                              size_t stream_stride, int reduce, bool want_c16, bool lean97, bool fuse_tail, uint8_t *lay, int layout,
                              void *data, size_t pitch, size_t plane_stride, size_t frame_stride, int rw, int rh)
{
    const int paw = c.aw >> reduce, pah = c.ah >> reduce;
    const size_t pp = (size_t)paw * (size_t)pah;
    if (int rc = decode_rgb_frames_reduced(go, c, a, w, n, streams, stream_stride, reduce, want_c16, lean97, fuse_tail, lay, lay + pp,
                                           lay + 2 * pp, 3ull * pp)) return rc;
    return emit_frames(go, layout, lay, 3 * pp, data, pitch, plane_stride, frame_stride, (int)n, rw, rh, paw, pah);
}

// ---- a probe of the quality calls (picsong_encode_frame_quality and its mirrors): the distortion of the nf coded arrays
// at q(j), without the coder -- it is lossless over the quantised coefficients, so the decoder's pixels follow from them:
//   quantise_kernel's int32 form over the unquantised float arrays (unit, unit_z bytes apart) into coef_i (P words each);
//   the synthesis at qs = q(j) with the DIVIDING kernels (fast = false: no per-qs verification of reciprocals, which
//   costs far more host time than the probe's GPU time; every reciprocal form is verified against these), grid.z = array,
//   work buffers of (P + extra) floats each, the clamped u8 pixels into `pix` (P bytes each);
//   sse_kernel against the input into out[0 .. nf).
// Grey (r == nullptr): nf frames at `frames`, frame_stride bytes apart.  RGB (nf = 3 n, n frames' planes frame_stride
// bytes after r / g / b): the components' planes leave the synthesis as float samples (the fused 9/7 RGB tail is the lean
// kernel's and wants the verified reciprocals: inv_rgb_tail_ok), component k of frame f in plane 3 f + k; then
//   rgb_sse_kernel: the inverse ICT and the SSE against the input planes in one launch, no pixel written, out[3 f + k];
//   or, where select_rgb_sse refuses (the float planes not 16-byte aligned, rgb_sse_fused = false: the library's
//   PICSONG_RGB_SSE_FUSED=0), the unfused tail: per frame the inverse ICT kernel writes R, G, B into pix (3 P bytes a
//   frame), each compared with its input plane by frames_sse.
// ssim (the SSIM calls, picsong_encode_frame_ssim and its mirrors): frames_dssim for frames_sse, out = DSSIM sums; an RGB
// probe takes the unfused tail whatever rgb_sse_fused says.
struct QualityProbe {
    const void *unit; unsigned long long unit_z;
    int32_t *coef_i; void *work; uint8_t *pix;
    int aw, ah, wl, w, h, off;
    size_t P, extra;
    int nf;
    const uint8_t *frames; size_t frame_stride;
    const uint8_t *r, *g, *b;
    bool rgb_sse_fused = true;
    bool ssim = false;              // the SSIM calls: out = DSSIM sums (frames_dssim); RGB on the unfused tail
};
// mark(k): called after the quantise pass (1), after the synthesis' last launch (2) and after the SSE (3) -- the
// library's stage timers; returns 0.  (RGB: the colour transform is in stage 2 on the unfused tail, in stage 3 on the
// fused one -- compare the two stages summed.)
struct NoMark { int operator()(int) const { return 0; } };
inline std::vector<InvLaunch> quality_probe_plan(const QualityProbe &p, int j, bool *pixels = nullptr)
{
    const bool rgb = p.r != nullptr;
    bool fused = false;
    std::vector<InvLaunch> plan = plan_inverse_frames(p.coef_i, p.work, rgb ? nullptr : p.pix, &fused, (unsigned)p.nf, p.P, false, rgb,
                                                      0, p.aw, p.ah, p.wl, rate_q(j), false, p.off, p.P, p.extra);
    if (pixels) *pixels = fused;
    return plan;
}
// the fused tail's launch over a probe's plan (kernel == nullptr: the unfused tail runs)
inline RgbSseLaunch quality_probe_rgb_sse(const QualityProbe &p, const std::vector<InvLaunch> &plan, unsigned long long *out, RgbSseArgs *args = nullptr)
{
    const RgbSseArgs s = rgb_sse_args(plan.back().a.dst, (unsigned long long)(p.P + p.extra) * 4ull, (size_t)p.aw, p.r, p.g, p.b,
                                      (unsigned long long)p.frame_stride, (size_t)p.aw, p.w, p.h, p.nf / 3, p.off, out);
    if (args) *args = s;
    return select_rgb_sse(s, p.rgb_sse_fused && !p.ssim);
}
// does an RGB probe over these buffers take the fused tail?  (else it needs p.pix: 3 P bytes a frame)
inline bool quality_probe_fuses(const QualityProbe &p)
{
    return p.r != nullptr && quality_probe_rgb_sse(p, quality_probe_plan(p, 1), nullptr).kernel != nullptr;
}
template <class Go, class Mark = NoMark>
int quality_probe(const Go &go, const QualityProbe &p, int j, unsigned long long *out, const Mark &mark = Mark())
{
    const bool rgb = p.r != nullptr;
    const bool forms[kQuantMaxK] = { false, false, false };
    const QuantArgs qa = quantise_args(p.unit, p.unit_z, p.coef_i, (unsigned long long)p.P * 4ull, p.aw, p.ah, p.wl, p.nf, 1, &j, forms);
    if (int rc = go(select_quantise(1, p.nf, p.ah, true).kernel, dim3(select_quantise(1, p.nf, p.ah, true).wgs), 256u, qa)) return rc;
    if (int rc = mark(1)) return rc;
    bool fused = false;
    const std::vector<InvLaunch> plan = quality_probe_plan(p, j, &fused);
    if (int rc = run_inverse(go, true, false, plan, (unsigned)p.nf)) return rc;
    const char *img = (const char *)plan.back().a.dst;       // (the finest level's samples where it did not write pixels)
    const size_t z = (p.P + p.extra) * 4;
    if (rgb) {
        const int n = p.nf / 3;
        RgbSseArgs sa;
        const RgbSseLaunch l = quality_probe_rgb_sse(p, plan, out, &sa);
        if (l.kernel) {
            if (int rc = mark(2)) return rc;
            if (int rc = go(sse_zero_kernel, dim3(1), 64u, out, p.nf)) return rc;
            if (int rc = go(l.kernel, dim3(l.wgs), 256u, sa)) return rc;
            return mark(3);
        }
        for (int f = 0; f < n; f++) {
            const char *c0 = img + (size_t)(3 * f) * z;
            uint8_t *px = p.pix + (size_t)(3 * f) * p.P;
            if (int rc = rgb_inverse(go, true, c0, c0 + z, c0 + 2 * z, px, px + p.P, px + 2 * p.P, p.P / 4, p.off)) return rc;
        }
        if (int rc = mark(2)) return rc;
        for (int f = 0; f < n; f++) {
            const size_t at = n > 1 ? (size_t)f * p.frame_stride : 0;
            const uint8_t *in[3] = { p.r + at, p.g + at, p.b + at };
            for (int k = 0; k < 3; k++)
                if (int rc = p.ssim ? frames_dssim(go, p.pix + (size_t)(3 * f + k) * p.P, (size_t)p.aw, 0, in[k], (size_t)p.aw, 0, p.w, p.h, 1, out + 3 * f + k)
                                    : frames_sse(go, p.pix + (size_t)(3 * f + k) * p.P, (size_t)p.aw, 0, in[k], (size_t)p.aw, 0, p.w, p.h, 1, out + 3 * f + k)) return rc;
        }
        return mark(3);
    }
    if (!fused)
        for (int f = 0; f < p.nf; f++)
            if (int rc = clamp_pixels(go, true, img + (size_t)f * z, p.pix + (size_t)f * p.P, p.P / 4, p.off)) return rc;
    if (int rc = mark(2)) return rc;
    if (p.ssim) {
        if (int rc = frames_dssim(go, p.pix, (size_t)p.aw, (unsigned long long)p.P, p.frames, (size_t)p.aw, (unsigned long long)p.frame_stride,
                                  p.w, p.h, p.nf, out)) return rc;
        return mark(3);
    }
    if (int rc = frames_sse(go, p.pix, (size_t)p.aw, (unsigned long long)p.P, p.frames, (size_t)p.aw, (unsigned long long)p.frame_stride,
                            p.w, p.h, p.nf, out)) return rc;
    return mark(3);
}

}  // namespace picsong
