// quality_kernels.hpp -- the distortion measurement of the quality calls (picsong_frames_sse,
// picsong_encode_frame_quality and its mirrors): the sum of squared differences of two u8 images.
//
// sse_kernel compares the VISIBLE W x H samples of n pairs of padded arrays -- each side with its own row pitch and its
// own frame stride -- and adds one uint64 per frame to out[f] (zeroed on the stream before it: sse_zero_kernel, the
// frames_sse sequence of launch_seq.hpp).  The sums are integers: exact, and the same from run to run whatever order
// the atomics land in.
//
// A bandwidth-bound stream shaped like quantise_kernel: 256 threads, 16 bytes a lane and load.  The work of a frame is
// its H * ceil(W / 16) vectors FLATTENED (an 8K row is 480 vectors: a row a pass would leave the second pass of 256
// lanes half empty), cut into tiles of kSseTileLoads loads a lane; tiles are dealt grid-stride over all frames, so a
// workgroup's frame only ever grows and it makes ONE 64-bit atomic add per frame it touched.  A lane divides once a
// tile (its first vector's row) and steps (row, vector) from there.
//
// The squares: sum (a - b)^2 = sum a^2 + sum b^2 - 2 sum a b, three v_dot4_u32_u8 per four samples with the
// accumulation in the instruction -- no unpacking, no per-byte |a - b| (which has no packed form on CDNA).  The two
// accumulators wrap modulo 2^32 on their own; their combination acc_sq - 2 acc_ab is the run's SSE modulo 2^32, so it
// is exact while the RUN's SSE stays below 2^32: one load adds at most 16 * 255^2 = 1 040 400, a run is at most
// kSseRunLoads = 4128 loads (4128 * 1 040 400 < 2^32 <= 4129 * 1 040 400), then the lane widens into its 64-bit sum.
// Samples outside the image -- the columns [W, pitch) in a row's last vector -- are masked to 0 on both sides per byte.
//
// VEC: both pointers, pitches and strides 16-byte aligned: dwordx4 loads.  Else the per-byte form: the same items, the
// sixteen bytes of a vector loaded one by one (bounds-checked against W), the same arithmetic.
//
// rgb_sse_kernel is the tail of an RGB quality probe (quality_probe, launch_seq.hpp): the inverse ICT of the float
// component planes the 9/7 synthesis leaves and the SSE against the caller's R, G, B planes in ONE pass -- the pixels are
// wanted for their squared error only, so none is written (the unfused tail, rgb_inverse_kernel and three sse_kernel
// launches, moves 21 P bytes a frame; this one reads 12 P of floats and 3 P of input).  out[3 f + c] += the SSE of plane c
// of frame f.  The pixel arithmetic is rgb_inverse_kernel<float>'s, bit for bit; the squares are sse_kernel's identity
// over the packed clamped pixels (3 v_lshl_or + 3 v_dot4 per four samples and channel against 4 byte extracts, 4
// subtracts and 4 multiply-adds unpacked); the shape is sse_kernel's with groups of four pixels for its vectors.
//
// ssim_kernel (at the end of this file, with its definition): the structural measure of the SSIM calls
// (picsong_frames_dssim, picsong_encode_frame_ssim and its mirrors) -- x264's integer 8 x 8 SSIM as a DSSIM sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dwt_kernels.hpp"

#ifndef __HIP_MEMORY_SCOPE_AGENT
#define __HIP_MEMORY_SCOPE_AGENT 4          // (CPU wave-emulator build: its atomics are plain read-modify-writes)
#endif

namespace picsong {

constexpr int kSseTileLoads = 4;            // loads a lane and tile
constexpr int kSseRunLoads = 4128;          // loads a lane may accumulate in 32 bits
constexpr unsigned kSseMaxWgs = 2048;       // 8 workgroups a CU
constexpr int kSseMaxFrames = 64;
static_assert(kSseRunLoads % kSseTileLoads == 0, "a run is whole tiles");
static_assert((unsigned long long)kSseRunLoads * 16ull * 255ull * 255ull < (1ull << 32), "a run's SSE fits 32 bits");

struct SseArgs {
    const uint8_t *a;               // frame f at a + f * a_z, row y at + y * a_pitch
    unsigned long long a_z;
    const uint8_t *b;
    unsigned long long b_z;
    unsigned long long *out;        // out[f] += the frame's sum
    uint32_t a_pitch, b_pitch;
    int W, H, n;
};

// c + the dot product of the four bytes of a and b (wraps modulo 2^32)
__device__ __forceinline__ uint32_t dot4_u8(uint32_t a, uint32_t b, uint32_t c)
{
#if defined(__HIP__)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else   // (CPU wave-emulator build)
    for (int i = 0; i < 4; i++) c += ((a >> (8 * i)) & 0xFFu) * ((b >> (8 * i)) & 0xFFu);
    return c;
#endif
}

__global__ __launch_bounds__(64) void sse_zero_kernel(unsigned long long *out, int n)
{
    for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) out[i] = 0ull;
}

template <bool VEC>
__global__ __launch_bounds__(256) void sse_kernel(SseArgs s)
{
    __shared__ unsigned long long wave_sum[4];
    const uint32_t vpr = ((uint32_t)s.W + 15u) >> 4;                        // vectors a row
    const uint32_t items = vpr * (uint32_t)s.H;                             // vectors a frame
    constexpr uint32_t kTile = 256u * (uint32_t)kSseTileLoads;
    const uint32_t tpf = (items + kTile - 1u) / kTile, tiles = tpf * (uint32_t)s.n;
    const uint32_t step_rows = 256u / vpr, step_vecs = 256u - step_rows * vpr;   // (row, vector) of item + 256
    const uint32_t tail = (uint32_t)s.W - 16u * (vpr - 1u);                 // visible bytes of a row's last vector, 1..16

    uint32_t acc_sq = 0u, acc_ab = 0u;                                      // the run: sum a^2 + b^2, sum a b
    int run = 0;
    unsigned long long sum = 0ull;
    uint32_t cur = tiles ? blockIdx.x / tpf : 0u;                           // the frame `sum` belongs to (workgroup-uniform)

    for (uint32_t t = blockIdx.x; ; t += gridDim.x) {
        const bool more = t < tiles;
        const uint32_t f = more ? t / tpf : cur + 1u;
        if (f != cur) {
            // ---- frame `cur` is done here: the waves reduce, the workgroup adds once
            sum += (unsigned long long)(acc_sq - 2u * acc_ab);
            acc_sq = acc_ab = 0u; run = 0;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
            if ((threadIdx.x & 63u) == 0u) wave_sum[threadIdx.x >> 6] = sum;
            __syncthreads();
            if (threadIdx.x == 0u) {
                const unsigned long long v = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
                if (v) (void)__hip_atomic_fetch_add(&s.out[cur], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
            sum = 0ull;
            cur = f;
        }
        if (!more) break;
        if (run + kSseTileLoads > kSseRunLoads) {                           // (uniform: every lane counts every tile)
            sum += (unsigned long long)(acc_sq - 2u * acc_ab);
            acc_sq = acc_ab = 0u; run = 0;
        }
        run += kSseTileLoads;
        const uint8_t *const fa = s.a + (unsigned long long)f * s.a_z;
        const uint8_t *const fb = s.b + (unsigned long long)f * s.b_z;
        uint32_t i = (t - f * tpf) * kTile + threadIdx.x;
        uint32_t y = i / vpr, v = i - y * vpr;
#pragma unroll
        for (int k = 0; k < kSseTileLoads; k++) {
            if (i < items) {
                const uint32_t rem = v == vpr - 1u ? tail : 16u;
                const size_t oa = (size_t)y * s.a_pitch + 16u * (size_t)v, ob = (size_t)y * s.b_pitch + 16u * (size_t)v;
                uint32_t wa[4], wb[4];
                if (VEC) {
                    const uint4 xa = *reinterpret_cast<const uint4 *>(fa + oa), xb = *reinterpret_cast<const uint4 *>(fb + ob);
                    wa[0] = xa.x; wa[1] = xa.y; wa[2] = xa.z; wa[3] = xa.w;
                    wb[0] = xb.x; wb[1] = xb.y; wb[2] = xb.z; wb[3] = xb.w;
                    if (rem < 16u) {
#pragma unroll
                        for (uint32_t d = 0; d < 4u; d++) {
                            const uint32_t m = rem >= 4u * d + 4u ? 0xFFFFFFFFu : (rem <= 4u * d ? 0u : (1u << (8u * (rem - 4u * d))) - 1u);
                            wa[d] &= m; wb[d] &= m;
                        }
                    }
                } else {
#pragma unroll
                    for (uint32_t d = 0; d < 4u; d++) {
                        wa[d] = wb[d] = 0u;
#pragma unroll
                        for (uint32_t e = 0; e < 4u; e++) {
                            if (4u * d + e < rem) {
                                wa[d] |= (uint32_t)fa[oa + 4u * d + e] << (8u * e);
                                wb[d] |= (uint32_t)fb[ob + 4u * d + e] << (8u * e);
                            }
                        }
                    }
                }
#pragma unroll
                for (int d = 0; d < 4; d++) {
                    acc_sq = dot4_u8(wa[d], wa[d], acc_sq);
                    acc_sq = dot4_u8(wb[d], wb[d], acc_sq);
                    acc_ab = dot4_u8(wa[d], wb[d], acc_ab);
                }
            }
            i += 256u; y += step_rows; v += step_vecs;
            if (v >= vpr) { v -= vpr; y++; }
        }
    }
}

// ---- inverse ICT + SSE of n RGB frames
constexpr int kRgbSseTileLoads = 4;         // groups of four pixels a lane and tile
constexpr int kRgbSseRunLoads = 16512;      // groups a lane may accumulate in 32 bits (a channel's sum)
static_assert(kRgbSseRunLoads % kRgbSseTileLoads == 0, "a run is whole tiles");

struct RgbSseArgs {
    const float *c;                 // component k of frame f: plane 3 f + k at c + (3 f + k) * c_z bytes, row y at + y * c_pitch floats
    unsigned long long c_z;
    const uint8_t *r, *g, *b;       // frame f's input planes at + f * in_z bytes, row y at + y * in_pitch
    unsigned long long in_z;
    unsigned long long *out;        // out[3 f + k] += the SSE of plane k of frame f
    uint32_t c_pitch, in_pitch;
    int W, H, n, off;
};

// RUN: the groups a lane accumulates before it widens (the library: kRgbSseRunLoads; the emulator test: two tiles).
// Wants c, c_z and c_pitch * 4 16-byte aligned, r, g, b, in_z and in_pitch 4-byte aligned (select_rgb_sse).
template <int RUN>
__global__ __launch_bounds__(256) void rgb_sse_kernel(RgbSseArgs s)
{
    static_assert(RUN >= kRgbSseTileLoads && RUN % kRgbSseTileLoads == 0, "a run is whole tiles");
    static_assert((unsigned long long)RUN * 4ull * 255ull * 255ull < (1ull << 32), "a run's SSE fits 32 bits");
    __shared__ unsigned long long wave_sum[3][4];
    const uint32_t gpr = ((uint32_t)s.W + 3u) >> 2;                         // groups a row
    const uint32_t items = gpr * (uint32_t)s.H;                             // groups a frame
    constexpr uint32_t kTile = 256u * (uint32_t)kRgbSseTileLoads;
    const uint32_t tpf = (items + kTile - 1u) / kTile, tiles = tpf * (uint32_t)s.n;
    const uint32_t step_rows = 256u / gpr, step_groups = 256u - step_rows * gpr;   // (row, group) of item + 256
    const uint32_t tail = (uint32_t)s.W - 4u * (gpr - 1u);                  // visible samples of a row's last group, 1..4
    const uint32_t tail_mask = tail >= 4u ? 0xFFFFFFFFu : (1u << (8u * tail)) - 1u;
    // rgb_inverse_kernel<float>'s matrix, the factors that are neither 0 nor 1 (from vector registers: rate_kernels.hpp)
    const float m02 = in_vgpr(1.402f), m11 = in_vgpr(-0.344136f), m12 = in_vgpr(-0.714136f), m21 = in_vgpr(1.772f);

    uint32_t acc_sq[3] = { 0u, 0u, 0u }, acc_ab[3] = { 0u, 0u, 0u };        // the run, per channel: sum a^2 + b^2, sum a b
    int run = 0;
    unsigned long long sum[3] = { 0ull, 0ull, 0ull };
    uint32_t cur = tiles ? blockIdx.x / tpf : 0u;                           // the frame `sum` belongs to (workgroup-uniform)

    for (uint32_t t = blockIdx.x; ; t += gridDim.x) {
        const bool more = t < tiles;
        const uint32_t f = more ? t / tpf : cur + 1u;
        if (f != cur) {
            // ---- frame `cur` is done here: the waves reduce, the workgroup adds once a channel
#pragma unroll
            for (int k = 0; k < 3; k++) {
                sum[k] += (unsigned long long)(acc_sq[k] - 2u * acc_ab[k]);
                acc_sq[k] = acc_ab[k] = 0u;
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) sum[k] += __shfl_xor(sum[k], m);
                if ((threadIdx.x & 63u) == 0u) wave_sum[k][threadIdx.x >> 6] = sum[k];
                sum[k] = 0ull;
            }
            run = 0;
            __syncthreads();
            if (threadIdx.x < 3u) {
                const unsigned long long v = wave_sum[threadIdx.x][0] + wave_sum[threadIdx.x][1] + wave_sum[threadIdx.x][2] +
                                             wave_sum[threadIdx.x][3];
                if (v) (void)__hip_atomic_fetch_add(&s.out[3u * cur + threadIdx.x], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
            cur = f;
        }
        if (!more) break;
        if (run + kRgbSseTileLoads > RUN) {                                 // (uniform: every lane counts every tile)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                sum[k] += (unsigned long long)(acc_sq[k] - 2u * acc_ab[k]);
                acc_sq[k] = acc_ab[k] = 0u;
            }
            run = 0;
        }
        run += kRgbSseTileLoads;
        const char *const fc = (const char *)s.c + (unsigned long long)(3u * f) * s.c_z;
        const float *const c0 = (const float *)fc, *const c1 = (const float *)(fc + s.c_z), *const c2 = (const float *)(fc + 2ull * s.c_z);
        const unsigned long long at = (unsigned long long)f * s.in_z;
        uint32_t i = (t - f * tpf) * kTile + threadIdx.x;
        uint32_t y = i / gpr, g = i - y * gpr;
#pragma unroll
        for (int l = 0; l < kRgbSseTileLoads; l++) {
            if (i < items) {
                const size_t oc = (size_t)y * s.c_pitch + 4u * (size_t)g, oi = at + (size_t)y * s.in_pitch + 4u * (size_t)g;
                const float4 vy = *reinterpret_cast<const float4 *>(c0 + oc), vb = *reinterpret_cast<const float4 *>(c1 + oc),
                             vr = *reinterpret_cast<const float4 *>(c2 + oc);
                const uint32_t mask = g == gpr - 1u ? tail_mask : 0xFFFFFFFFu;
                const uint32_t in[3] = { *reinterpret_cast<const uint32_t *>(s.r + oi) & mask, *reinterpret_cast<const uint32_t *>(s.g + oi) & mask,
                                         *reinterpret_cast<const uint32_t *>(s.b + oi) & mask };
                const float py[4] = { vy.x, vy.y, vy.z, vy.w }, pb[4] = { vb.x, vb.y, vb.z, vb.w }, pr[4] = { vr.x, vr.y, vr.z, vr.w };
                uint32_t px[3] = { 0u, 0u, 0u };
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float yy = py[e], cb = pb[e], cr = pr[e];
                    const int R = (int)rintf(fmaf(m02, cr, fmaf(0.0f, cb, 1.0f * yy)) + 0.01f);
                    const int G = (int)rintf(fmaf(m12, cr, fmaf(m11, cb, 1.0f * yy)) + 0.01f);
                    const int B = (int)rintf(fmaf(0.0f, cr, fmaf(m21, cb, 1.0f * yy)) + 0.01f);
                    px[0] |= clamp_u8(R + s.off) << (8 * e);
                    px[1] |= clamp_u8(G + s.off) << (8 * e);
                    px[2] |= clamp_u8(B + s.off) << (8 * e);
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const uint32_t p = px[k] & mask;
                    acc_sq[k] = dot4_u8(p, p, acc_sq[k]);
                    acc_sq[k] = dot4_u8(in[k], in[k], acc_sq[k]);
                    acc_ab[k] = dot4_u8(p, in[k], acc_ab[k]);
                }
            }
            i += 256u; y += step_rows; g += step_groups;
            if (g >= gpr) { g -= gpr; y++; }
        }
    }
}

// ---- structural similarity of n pairs of u8 frames (picsong_frames_dssim, the -ssim search calls' probes)
// The measure is x264 / ffmpeg's integer 8 x 8 SSIM over the VISIBLE W x H samples (W, H >= 8): windows of 8 x 8 samples
// at the origins (4 x, 4 y), x < nx = (W - 8) / 4 + 1, y < ny = (H - 8) / 4 + 1; a window's exact integer sums
//   s1 = sum a, s2 = sum b, ss = sum a^2 + sum b^2, s12 = sum a b      (64 samples)
// give, with c1 = 416 and c2 = 235963,
//   A = 2 s1 s2 + c1, B = 2 (64 s12 - s1 s2) + c2, C = s1^2 + s2^2 + c1, E = 64 ss - s1^2 - s2^2 + c2   (each below 2^30)
//   v = ((double)A * (double)B) / ((double)C * (double)E)   -- three IEEE double operations, a true division, and no
//   addition a product could contract into;  q = (int64)floor(v * 2^24) <= 2^24, negative for anti-correlated content.
// out[f] += sum over frame f's windows of (2^24 - q): the DSSIM sum nx ny 2^24 - sum q, formed HERE window by window so
// that every partial sum is a non-negative integer -- exact, and the same whatever order the atomics land in.
//
// Shape: a window is four 4 x 4 blocks.  A lane owns a block COLUMN: per sample row one dword of each image, the block's
// four sums accumulated by five v_dot4_u32_u8 a row (sum a and sum b as dots with 0x01010101) -- each image byte is
// loaded once but for the overlaps below, the traffic of sse_kernel.  After a block row the lane adds its LEFT
// neighbour's block (wave_shr:1) for the pair sums of the window whose right half it owns; the previous block row's pair
// sums stay in registers as the band streams down, so a window is pair(y) + pair(y + 1).  A wave takes a strip of 64
// block columns = kSsimStripWindows = 63 window columns (lane 0's window would need the block left of the strip: strips
// overlap by one block column) over a band of kSsimBandWindows window rows (kSsimBandWindows + 1 block rows: bands overlap
// by one block row).  Window (x, y) is counted by the one strip with x / 63 and the one band with y / 16: exactly once.
// Every block a window uses lies inside the visible part (4 (nx + 1) <= W): nothing is masked; the columns from
// 4 (nx + 1) and the rows from 4 (ny + 1) on belong to no window and are not read.
// The (strip, band) items of a frame are dealt four a tile to a workgroup's four waves, tiles grid-stride over all frames
// as sse_kernel's: a workgroup's frame only grows, and it makes ONE 64-bit atomic add per frame it touched.
//
// VEC: both pointers, pitches and strides 4-byte aligned: dword loads.  Else the per-byte form: the same items, a
// block row's four bytes loaded one by one, the same arithmetic.
constexpr int kSsimStripWindows = 63;       // window columns a wave
constexpr int kSsimBandWindows = 16;        // window rows a wave item
constexpr int kSsimC1 = 416, kSsimC2 = 235963;

// 2^24 - q of a window with the sums s1, s2, ss, s12
__device__ __forceinline__ unsigned long long ssim_window_d(uint32_t s1, uint32_t s2, uint32_t ss, uint32_t s12)
{
    const int p12 = (int)(s1 * s2), sq = (int)(s1 * s1 + s2 * s2);         // <= 2 * 16320^2 < 2^30
    const int vars = (int)(64u * ss) - sq, cov = (int)(64u * s12) - p12;
    const double num = (double)(2 * p12 + kSsimC1) * (double)(2 * cov + kSsimC2);
    const double den = (double)(sq + kSsimC1) * (double)(vars + kSsimC2);
    const double v = num / den;
    const long long q = (long long)floor(v * 16777216.0);
    return (unsigned long long)(16777216ll - q);
}

template <bool VEC>
__global__ __launch_bounds__(256) void ssim_kernel(SseArgs s)
{
    __shared__ unsigned long long wave_sum[4];
    const uint32_t nx = ((uint32_t)s.W - 8u) / 4u + 1u, ny = ((uint32_t)s.H - 8u) / 4u + 1u;
    const uint32_t strips = (nx + (uint32_t)kSsimStripWindows - 1u) / (uint32_t)kSsimStripWindows;
    const uint32_t bands = (ny + (uint32_t)kSsimBandWindows - 1u) / (uint32_t)kSsimBandWindows;
    const uint32_t ipf = strips * bands;                                    // wave items a frame
    const uint32_t tpf = (ipf + 3u) / 4u, tiles = tpf * (uint32_t)s.n;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;

    unsigned long long sum = 0ull;
    uint32_t cur = tiles ? blockIdx.x / tpf : 0u;                           // the frame `sum` belongs to (workgroup-uniform)

    for (uint32_t t = blockIdx.x; ; t += gridDim.x) {
        const bool more = t < tiles;
        const uint32_t f = more ? t / tpf : cur + 1u;
        if (f != cur) {
            // ---- frame `cur` is done here: the waves reduce, the workgroup adds once
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
            if (lane == 0u) wave_sum[wave] = sum;
            __syncthreads();
            if (threadIdx.x == 0u) {
                const unsigned long long v = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
                if (v) (void)__hip_atomic_fetch_add(&s.out[cur], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
            sum = 0ull;
            cur = f;
        }
        if (!more) break;
        const uint32_t i = (t - f * tpf) * 4u + wave;                       // (wave-uniform)
        if (i >= ipf) continue;
        const uint32_t band = i / strips, strip = i - band * strips;
        const uint32_t bx = strip * (uint32_t)kSsimStripWindows + lane;     // the lane's block column
        const bool have = bx <= nx;                                         // block columns 0 .. nx carry windows
        const bool win = have && lane != 0u;                                // window bx - 1: the left block is lane - 1's
        const uint32_t by0 = band * (uint32_t)kSsimBandWindows;             // block rows by0 .. by1
        const uint32_t by1 = by0 + (uint32_t)kSsimBandWindows < ny ? by0 + (uint32_t)kSsimBandWindows : ny;
        const uint8_t *pa = s.a + (unsigned long long)f * s.a_z + (size_t)(4u * by0) * s.a_pitch + 4u * (size_t)bx;
        const uint8_t *pb = s.b + (unsigned long long)f * s.b_z + (size_t)(4u * by0) * s.b_pitch + 4u * (size_t)bx;
        uint32_t u1 = 0u, u2 = 0u, uss = 0u, u12 = 0u;                      // the pair sums of the block row above
        for (uint32_t by = by0; by <= by1; by++) {
            uint32_t b1 = 0u, b2 = 0u, bss = 0u, b12 = 0u;                  // the lane's block
            if (have) {
                uint32_t wa[4], wb[4];
#pragma unroll
                for (uint32_t r = 0; r < 4u; r++) {
                    const uint8_t *const ra = pa + (size_t)r * s.a_pitch, *const rb = pb + (size_t)r * s.b_pitch;
                    if (VEC) {
                        wa[r] = *reinterpret_cast<const uint32_t *>(ra);
                        wb[r] = *reinterpret_cast<const uint32_t *>(rb);
                    } else {
                        wa[r] = (uint32_t)ra[0] | (uint32_t)ra[1] << 8 | (uint32_t)ra[2] << 16 | (uint32_t)ra[3] << 24;
                        wb[r] = (uint32_t)rb[0] | (uint32_t)rb[1] << 8 | (uint32_t)rb[2] << 16 | (uint32_t)rb[3] << 24;
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    b1 = dot4_u8(wa[r], 0x01010101u, b1);
                    b2 = dot4_u8(wb[r], 0x01010101u, b2);
                    bss = dot4_u8(wa[r], wa[r], bss);
                    bss = dot4_u8(wb[r], wb[r], bss);
                    b12 = dot4_u8(wa[r], wb[r], b12);
                }
            }
            // the pair (bx - 1, bx) of this block row (wave_shr:1; lane 0 reads 0 and has no window)
            const uint32_t h1 = b1 + __builtin_amdgcn_update_dpp(0u, b1, 0x138, 0xf, 0xf, true);
            const uint32_t h2 = b2 + __builtin_amdgcn_update_dpp(0u, b2, 0x138, 0xf, 0xf, true);
            const uint32_t hss = bss + __builtin_amdgcn_update_dpp(0u, bss, 0x138, 0xf, 0xf, true);
            const uint32_t h12 = b12 + __builtin_amdgcn_update_dpp(0u, b12, 0x138, 0xf, 0xf, true);
            if (win && by != by0) sum += ssim_window_d(u1 + h1, u2 + h2, uss + hss, u12 + h12);   // window (bx - 1, by - 1)
            u1 = h1; u2 = h2; uss = hss; u12 = h12;
            pa += 4u * (size_t)s.a_pitch; pb += 4u * (size_t)s.b_pitch;
        }
    }
}

}  // namespace picsong
