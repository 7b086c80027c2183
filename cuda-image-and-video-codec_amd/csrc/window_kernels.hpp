// window_kernels.hpp -- the synthesis of a window's dependency cone (picsong_decode_frame_window and its mirrors; no
// reference counterpart), one level a launch, for gfx950 and the CPU wave emulator.
//
// Level l computes LL_l over the rectangle R_l of window_plan (launch_plan.hpp) only.  It reads LL_{l+1} over R_{l+1}
// (the previous launch's compact rectangle, or the Mallat array at l = wl - 1) and HL / LH / HH over S_l from the
// Mallat array.  A workgroup owns a kWinTile x kWinTile tile of R_l and builds in LDS the interleaved samples of the
// tile plus a halo of 2 (5/3) or 4 (9/7) samples a side -- the radius of the 2 / 4 lifting steps.  Halo samples outside
// LL_l come from their mirror position (reflect's whole-sample symmetric extension, folded twice: a level may be 4
// samples wide and the 9/7 halo is 4), so every lifting step runs the interior formula on every tile sample and the
// samples in LL_l are those of whole-image lifting: the oracle's edges (x[-1] = x[1], x[n] = x[n-2]) included.
// The lifting runs in the oracle's order (po_53_inv_1d / po_97_inv_1d): horizontal over all the tile's rows, then
// vertical, a barrier between steps.  9/7 divides as the oracle does -- ((m * s) / q) / qs on the read, x / N1 and
// x / N2 with true divisions (div_n1<true>, div_n2<true>), explicit fmaf in po_97_inv_1d's operation order.
// Intermediate levels store R_l as T (row stride its width); level r stores pixels into the caller's window through
// to_pixel (grey; a deep context: uint16 samples through to_sample16), or T that window_rgb_kernel turns into the three
// pixel planes (RGB; n frames in any colour layout: window_rgb_image_kernel; a deep RGB context: window_rgb16_image_kernel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "bpc_kernels.hpp"
#include "dwt_kernels.hpp"
#include "launch_plan.hpp"
#include "layout_kernels.hpp"

namespace picsong {

constexpr int kWinTile = 64;            // output samples per tile side; 256 threads a workgroup
// what a level stores: T over its rectangle, or -- level r of a grey call -- the window's u8 pixels or uint16 samples
constexpr int kWinOutT = 0, kWinOutU8 = 1, kWinOutU16 = 2;

struct WinSynArgs {
    const int32_t *mallat;              // the decoder's int32 Mallat array, row stride AW
    int AW;
    const void *ll;                     // LL_{l+1} over R_{l+1}: T, row stride ll_stride, its origin at (ll_x0, ll_y0)
    int ll_x0, ll_y0, ll_stride;
    int first;                          // l = wl - 1: LL_wl is read (and de-quantised) from the Mallat array instead
    int W, H;                           // LL_l's size
    int x0, y0, x1, y1;                 // R_l
    void *dst;                          // kWinOutT: T over R_l, row stride x1 - x0
    uint8_t *dst_u8;                    // kWinOutU8: the window's pixels, row (y - y0) at dst_u8 + (y - y0) * pitch;
                                        // kWinOutU16: its uint16 samples, the same row address (pitch in bytes, even)
    unsigned long long pitch;
    int off;                            // level shift
    float qs, q[4];                     // 9/7: the quantisation steps of level l (LL, HL, LH, HH) and the context's qs
    // grid.z = frames of a batched call (or the components of an RGB frame): frame z reads mallat + z * mallat_z and
    // ll + z * ll_z, writes dst + z * dst_z and dst_u8 + z * u8_z (bytes)
    unsigned long long mallat_z, ll_z, dst_z, u8_z;
    int px_max;                         // kWinOutU16: the samples are clamped to [0, px_max]  (last: the fields above keep their offsets)
};

// reflect() folded twice (see above); i in [-4, n + 3], n >= 4
__device__ __forceinline__ int win_mirror(int i, int n)
{
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (i < 0) i = -i;
        if (i >= n) i = 2 * (n - 1) - i;
    }
    return i;
}

// one lifting step of po_53_inv_1d / po_97_inv_1d on sample x with neighbours p (before) and n (after).
// 5/3: STEP 0 the even update, 1 the odd prediction.  9/7: STEP 0..3 = A4 (even), A3 (odd), A2 (even), A1 (odd).
template <int STEP> __device__ __forceinline__ int win_lift(int x, int p, int n)
{
    if constexpr (STEP == 0) return x - ((p + n + 2) >> 2);
    else return x + ((p + n) >> 1);
}
template <int STEP> __device__ __forceinline__ float win_lift(float x, float p, float n)
{
    constexpr float A = STEP == 0 ? PS_A4 : (STEP == 1 ? PS_A3 : (STEP == 2 ? PS_A2 : PS_A1));
    return fmaf(-(p + n), A, x);
}

// STEP over the tile's samples of its parity (even steps: even coordinates), horizontally (along rows) or vertically.
// Tile sample (i, j) is LL_l's (gx0 + i, gy0 + j); nx x ny samples in use, row stride TS.  The tile's outer samples
// have no neighbour on one side and are left as they are: each step shrinks the exact region by one, the halo by as many.
template <typename T, int STEP, bool HORIZ, int TS>
__device__ __forceinline__ void win_step(T *tile, int nx, int ny, int gx0, int gy0)
{
    constexpr int par = STEP & 1;
    if constexpr (HORIZ) {
        const int i0 = 1 + (((gx0 + 1) & 1) ^ par);          // first i >= 1 with (gx0 + i) & 1 == par
        const int half = (nx - 1 - i0 + 1) / 2;               // i = i0, i0 + 2, ... < nx - 1
        for (int j = (int)threadIdx.x >> 5; j < ny; j += 8)
            for (int k = (int)threadIdx.x & 31; k < half; k += 32) {
                T *p = tile + j * TS + i0 + 2 * k;
                p[0] = win_lift<STEP>(p[0], p[-1], p[1]);
            }
    } else {
        const int j0 = 1 + (((gy0 + 1) & 1) ^ par);
        const int half = (ny - 1 - j0 + 1) / 2;
        for (int k = (int)threadIdx.x >> 6; k < half; k += 4)
            for (int i = (int)threadIdx.x & 63; i < nx; i += 64) {
                T *p = tile + (j0 + 2 * k) * TS + i;
                p[0] = win_lift<STEP>(p[0], p[-TS], p[TS]);
            }
    }
    __syncthreads();
}

// T = int (5/3) or float (9/7); OUT: kWinOutT, or level r of a grey call -- kWinOutU8: pixels into the window, kWinOutU16
// (a deep context): uint16 samples into it, rows a.pitch BYTES apart
template <typename T, int OUT>
__global__ __launch_bounds__(256) void dwt_window_kernel(WinSynArgs a)
{
    constexpr bool LOSSY = std::is_same<T, float>::value;
    constexpr int HL = LOSSY ? 4 : 2;                        // halo: the lifting steps of a direction
    constexpr int TS = kWinTile + 2 * HL;
    __shared__ T tile[TS * TS];
    {
        const unsigned long long z = blockIdx.z;
        a.mallat = (const int32_t *)((const char *)a.mallat + z * a.mallat_z);
        a.ll = (const char *)a.ll + z * a.ll_z;
        a.dst = (char *)a.dst + z * a.dst_z;
        if (OUT != kWinOutT) a.dst_u8 += z * a.u8_z;
    }
    const int tx0 = a.x0 + (int)blockIdx.x * kWinTile, ty0 = a.y0 + (int)blockIdx.y * kWinTile;
    const int tw = imin(kWinTile, a.x1 - tx0), th = imin(kWinTile, a.y1 - ty0);
    const int gx0 = tx0 - HL, gy0 = ty0 - HL;               // LL_l coordinates of tile sample (0, 0)
    const int nx = tw + 2 * HL, ny = th + 2 * HL;
    const int hW = a.W >> 1, hH = a.H >> 1;

    // ---- load: the interleaved samples, mirrored where outside LL_l; 9/7 takes the horizontal pass's divisions here
    // (x / N1 on odd columns, x / N2 on even ones: po_97_inv_1d's first operations on a sample, pointwise)
    for (int j = (int)threadIdx.x >> 6; j < ny; j += 4) {
        const int gy = win_mirror(gy0 + j, a.H);
        const int n = gy >> 1, by = gy & 1;
        for (int i = (int)threadIdx.x & 63; i < nx; i += 64) {
            const int gx = win_mirror(gx0 + i, a.W);
            const int m = gx >> 1, bx = gx & 1;
            T v;
            if (!bx && !by && !a.first) {
                v = reinterpret_cast<const T *>(a.ll)[(size_t)(n - a.ll_y0) * (size_t)a.ll_stride + (size_t)(m - a.ll_x0)];
            } else {
                const int32_t c = a.mallat[(size_t)(n + by * hH) * (size_t)a.AW + (size_t)(m + bx * hW)];
                if constexpr (LOSSY) {
                    const float q = by ? (bx ? a.q[3] : a.q[2]) : (bx ? a.q[1] : a.q[0]);
                    v = dequant<false>(c, q, 0.0f, a.qs, 0.0f);
                } else {
                    v = c;
                }
            }
            if constexpr (LOSSY) v = bx ? div_n1<true>(v) : div_n2<true>(v);
            tile[j * TS + i] = v;
        }
    }
    __syncthreads();

    // ---- horizontal, every row of the tile
    if constexpr (LOSSY) {
        win_step<T, 0, true, TS>(tile, nx, ny, gx0, gy0);
        win_step<T, 1, true, TS>(tile, nx, ny, gx0, gy0);
        win_step<T, 2, true, TS>(tile, nx, ny, gx0, gy0);
        win_step<T, 3, true, TS>(tile, nx, ny, gx0, gy0);
        // the vertical pass's divisions, pointwise: x / N1 on odd rows, x / N2 on even ones
        for (int j = (int)threadIdx.x >> 6; j < ny; j += 4) {
            const bool odd = ((gy0 + j) & 1) != 0;
            for (int i = (int)threadIdx.x & 63; i < nx; i += 64) {
                T &v = tile[j * TS + i];
                v = odd ? div_n1<true>(v) : div_n2<true>(v);
            }
        }
        __syncthreads();
        win_step<T, 0, false, TS>(tile, nx, ny, gx0, gy0);
        win_step<T, 1, false, TS>(tile, nx, ny, gx0, gy0);
        win_step<T, 2, false, TS>(tile, nx, ny, gx0, gy0);
        win_step<T, 3, false, TS>(tile, nx, ny, gx0, gy0);
    } else {
        win_step<T, 0, true, TS>(tile, nx, ny, gx0, gy0);
        win_step<T, 1, true, TS>(tile, nx, ny, gx0, gy0);
        win_step<T, 0, false, TS>(tile, nx, ny, gx0, gy0);
        win_step<T, 1, false, TS>(tile, nx, ny, gx0, gy0);
    }

    // ---- store the tile's own samples
    const int ox = tx0 - a.x0, oy = ty0 - a.y0, ow = a.x1 - a.x0;
    for (int j = (int)threadIdx.x >> 6; j < th; j += 4)
        for (int i = (int)threadIdx.x & 63; i < tw; i += 64) {
            const T v = tile[(j + HL) * TS + i + HL];
            if constexpr (OUT == kWinOutU8) a.dst_u8[(size_t)(oy + j) * a.pitch + (size_t)(ox + i)] = (uint8_t)to_pixel(v, a.off);
            else if constexpr (OUT == kWinOutU16)
                reinterpret_cast<uint16_t *>(a.dst_u8 + (size_t)(oy + j) * a.pitch)[(size_t)(ox + i)] = (uint16_t)to_sample16(v, a.off, a.px_max);
            else reinterpret_cast<T *>(a.dst)[(size_t)(oy + j) * (size_t)ow + (size_t)(ox + i)] = v;
        }
}

// The inverse RCT / ICT of one pixel's three component samples, level shift and clamp -- rgb_inverse_kernel's arithmetic
template <typename T>
__device__ __forceinline__ void window_rgb_px(T yy, T cb, T cr, int off, uint32_t &r, uint32_t &g, uint32_t &b)
{
    int R, G, B;
    if constexpr (std::is_integral<T>::value) {
        G = (int)yy - (((int)cb + (int)cr) >> 2);
        R = (int)cr + G;
        B = (int)cb + G;
    } else {
        const float M[3][3] = { { 1.0f, 0.0f, 1.402f }, { 1.0f, -0.344136f, -0.714136f }, { 1.0f, 1.772f, 0.0f } };
        R = (int)rintf(fmaf(M[0][2], cr, fmaf(M[0][1], cb, M[0][0] * yy)) + 0.01f);
        G = (int)rintf(fmaf(M[1][2], cr, fmaf(M[1][1], cb, M[1][0] * yy)) + 0.01f);
        B = (int)rintf(fmaf(M[2][2], cr, fmaf(M[2][1], cb, M[2][0] * yy)) + 0.01f);
    }
    r = (uint32_t)clamp_u8(R + off);
    g = (uint32_t)clamp_u8(G + off);
    b = (uint32_t)clamp_u8(B + off);
}

// RGB window calls, one frame into planar planes (decode_rgb_frames, launch_seq.hpp): the inverse RCT / ICT of the three
// components' level-r samples (compact, w x h, row stride w, the components z_stride bytes apart), level shift and clamp
// into the three pixel planes, row i at r / g / b + i * pitch
template <typename T>
__global__ __launch_bounds__(256) void window_rgb_kernel(const T *c0, unsigned long long z_stride, int w, int h, uint8_t *r,
                                                         uint8_t *g, uint8_t *b, unsigned long long pitch, int off)
{
    const T *c1 = (const T *)((const char *)c0 + z_stride), *c2 = (const T *)((const char *)c0 + 2 * z_stride);
    const int y = (int)blockIdx.y;
    for (int x = (int)(blockIdx.x * blockDim.x + threadIdx.x); x < w; x += (int)(gridDim.x * blockDim.x)) {
        const size_t i = (size_t)y * (size_t)w + (size_t)x;
        uint32_t R, G, B;
        window_rgb_px<T>(c0[i], c1[i], c2[i], off, R, G, B);
        const size_t o = (size_t)y * (size_t)pitch + (size_t)x;
        r[o] = (uint8_t)R;
        g[o] = (uint8_t)G;
        b[o] = (uint8_t)B;
    }
}

// The epilogue of every other RGB window call (n frames, or an interleaved layout: picsong_decode_rgb_frames_window,
// picsong_decode_rgb_images_window and _reduced): the same arithmetic over the w x h windows of n frames, grid.z = frame,
// stored in the caller's pixel layout -- kLayoutPlanar3 (three plane pointers) or an interleaved layout of
// layout_kernels.hpp, alpha 255.  There is no planar intermediate and no emit pass.
//   A thread converts four adjacent pixels of a row: it reads 3 x 16 bytes (one dwordx4 a component where the source rows
//   are 16-byte aligned: w a multiple of 4) and stores one dword a plane, three dwords (RGB24 / BGR24, repacked with
//   byte permutes: layout_store_vec) or 16 bytes (RGBA32 / BGRA32; one dwordx4 where a16).  Threads run along the rows of
//   the window, row after row, so a narrow window still fills its waves; the kernel holds no LDS and few registers, its
//   occupancy is the grid's.
//   VEC: every store address is 4-byte aligned (pointers, pitch, frame stride).  The row's last, partial group and every
//   destination that is not so aligned are stored per byte; the bytes are the same.  No byte outside
//   [i * pitch, i * pitch + w * bpp) of rows 0 .. h - 1 is written.
struct WinRgbArgs {
    const void *work;                   // frame z's component c: T[w * h], row stride w, at work + (3 z + c) * z_stride
    unsigned long long z_stride;
    int w, h;
    int src16;                          // the component rows take dwordx4 loads
    uint8_t *dst[3];                    // frame 0 -- planar: the R, G, B planes; interleaved: dst[0], the pixels
    unsigned long long pitch, frame_stride;
    int off;                            // level shift
    int a16;                            // VEC: the destination is 16-byte aligned as well
};

template <typename T>
__device__ __forceinline__ void win_load4(const T *p, bool vec, uint32_t nvis, T (&v)[4])
{
    if (vec) {
        const uint4 q = *reinterpret_cast<const uint4 *>(p);
        const uint32_t w[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if constexpr (std::is_integral<T>::value) v[k] = (T)(int)w[k];
            else v[k] = __uint_as_float(w[k]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = (uint32_t)k < nvis ? p[k] : (T)0;
    }
}

template <typename T, int L, bool VEC>
__global__ __launch_bounds__(256) void window_rgb_image_kernel(WinRgbArgs a)
{
    using LT = LayoutTraits<L>;
    static_assert(L == kLayoutPlanar3 || LT::inter, "a colour layout");
    const uint32_t w = (uint32_t)a.w, gpr = (w + 3u) / 4u;                  // groups of four pixels a row
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= gpr * (uint32_t)a.h) return;
    const uint32_t y = t / gpr, x0 = (t - y * gpr) * 4u, nvis = w - x0 < 4u ? w - x0 : 4u;
    const unsigned long long z = blockIdx.z;
    const char *const src = (const char *)a.work + 3ull * z * a.z_stride;
    const size_t i = (size_t)y * (size_t)w + (size_t)x0;
    T c[3][4];
#pragma unroll
    for (int k = 0; k < 3; k++) win_load4<T>((const T *)(src + (unsigned long long)k * a.z_stride) + i, a.src16 != 0, nvis, c[k]);
    uint32_t p[3][1] = { { 0u }, { 0u }, { 0u } };                          // four pixels of R, G, B, a byte each
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t R, G, B;
        window_rgb_px<T>(c[0][k], c[1][k], c[2][k], a.off, R, G, B);
        p[0][0] |= R << (8 * k); p[1][0] |= G << (8 * k); p[2][0] |= B << (8 * k);
    }
    const size_t row = (size_t)z * a.frame_stride + (size_t)y * a.pitch;
    if constexpr (!LT::inter) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            uint8_t *const q = a.dst[k] + row + x0;
            if (VEC && nvis == 4u) {
                *reinterpret_cast<uint32_t *>(q) = p[k][0];
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 4u; j++)
                    if (j < nvis) q[j] = (uint8_t)(p[k][0] >> (8u * j));
            }
        }
    } else {
        uint8_t *const q = a.dst[0] + row + (size_t)x0 * LT::bpp;
        if (VEC && nvis == 4u) {
            layout_store_vec<L>(q, a.a16 != 0, p);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                if (j < nvis) {
#pragma unroll
                    for (int k = 0; k < 3; k++) q[j * LT::bpp + layout_chan<L>(k)] = (uint8_t)(p[k][0] >> (8u * j));
                    if (LT::bpp == 4) q[j * LT::bpp + 3u] = 0xFFu;
                }
            }
        }
    }
}

// The epilogue of the deep RGB window calls (picsong_decode_rgb_frames16_window, picsong_decode_rgb_images_window and
// _reduced on a deep RGB context): the same walk -- a thread four adjacent pixels of a row, threads along the rows of the
// window, row after row, grid.z = frame, 3 x 16 bytes read, no LDS -- with rgb_inverse16_kernel's arithmetic
// (rgb_inverse16_px: level shift `off`, clamp to [0, mx]) and uint16 samples stored in kLayoutPlanar3_16 (8 bytes a
// plane), kLayoutRgb48 (24 bytes) or kLayoutRgba64 (32 bytes, alpha = mx).  Pitch and frame stride in bytes.
//   VEC: every store address is 4-byte aligned (pointers, pitch, frame stride): dword stores, or -- a8: all of them 8-byte
//   aligned as well -- dwordx2 ones; a thread's bytes are contiguous and so are a wave's, 512 / 1536 / 2048 bytes a row
//   segment.  The row's last, partial group and every destination that is not so aligned are stored sample by sample; the
//   bytes are the same.  No byte outside [i * pitch, i * pitch + w * bpp) of rows 0 .. h - 1 is written.
struct WinRgb16Args {
    const void *work;                   // frame z's component c: T[w * h], row stride w, at work + (3 z + c) * z_stride
    unsigned long long z_stride;
    int w, h;
    int src16;                          // the component rows take dwordx4 loads
    uint8_t *dst[3];                    // frame 0 -- planar: the R, G, B planes; interleaved: dst[0], the pixels
    unsigned long long pitch, frame_stride;
    int off, mx;                        // level shift, 2^(bit depth) - 1
    int a8;                             // VEC: the destination is 8-byte aligned as well
};

template <int L> struct WinRgb16Traits {
    static_assert(L == kLayoutPlanar3_16 || L == kLayoutRgb48 || L == kLayoutRgba64, "a 16-bit colour layout");
    static constexpr bool inter = L != kLayoutPlanar3_16;
    static constexpr int spp = L == kLayoutRgba64 ? 4 : 3;               // samples a pixel (interleaved)
};

// ND dwords to q (4-byte aligned; a8: 8-byte aligned, ND even)
template <int ND>
__device__ __forceinline__ void win_store_dwords(uint8_t *q, bool a8, const uint32_t (&d)[ND])
{
    static_assert(ND % 2 == 0, "whole dwordx2");
    if (a8) {
#pragma unroll
        for (int k = 0; k < ND / 2; k++) {
            uint2 v;
            v.x = d[2 * k]; v.y = d[2 * k + 1];
            reinterpret_cast<uint2 *>(q)[k] = v;
        }
    } else {
#pragma unroll
        for (int k = 0; k < ND; k++) reinterpret_cast<uint32_t *>(q)[k] = d[k];
    }
}

template <typename T, int L, bool VEC>
__global__ __launch_bounds__(256) void window_rgb16_image_kernel(WinRgb16Args a)
{
    using LT = WinRgb16Traits<L>;
    const uint32_t w = (uint32_t)a.w, gpr = (w + 3u) / 4u;                  // groups of four pixels a row
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= gpr * (uint32_t)a.h) return;
    const uint32_t y = t / gpr, x0 = (t - y * gpr) * 4u, nvis = w - x0 < 4u ? w - x0 : 4u;
    const unsigned long long z = blockIdx.z;
    const char *const src = (const char *)a.work + 3ull * z * a.z_stride;
    const size_t i = (size_t)y * (size_t)w + (size_t)x0;
    T c[3][4];
#pragma unroll
    for (int k = 0; k < 3; k++) win_load4<T>((const T *)(src + (unsigned long long)k * a.z_stride) + i, a.src16 != 0, nvis, c[k]);
    uint32_t s[3][4];                                                       // four pixels of R, G, B, a sample each
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t q[3];
#pragma unroll
        for (int m = 0; m < 3; m++) {
            if constexpr (std::is_integral<T>::value) q[m] = (uint32_t)c[m][k];
            else q[m] = __float_as_uint(c[m][k]);
        }
        rgb_inverse16_px<T>(q[0], q[1], q[2], a.off, a.mx, s[0][k], s[1][k], s[2][k]);
    }
    const size_t row = (size_t)z * a.frame_stride + (size_t)y * a.pitch;
    if constexpr (!LT::inter) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            uint8_t *const q = a.dst[k] + row + (size_t)x0 * 2u;
            if (VEC && nvis == 4u) {
                const uint32_t d[2] = { s[k][0] | (s[k][1] << 16), s[k][2] | (s[k][3] << 16) };
                win_store_dwords<2>(q, a.a8 != 0, d);
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 4u; j++)
                    if (j < nvis) reinterpret_cast<uint16_t *>(q)[j] = (uint16_t)s[k][j];
            }
        }
    } else {
        uint8_t *const q = a.dst[0] + row + (size_t)x0 * (2u * LT::spp);
        if (VEC && nvis == 4u) {
            if constexpr (LT::spp == 3) {
                // r0 g0 | b0 r1 | g1 b1 | r2 g2 | b2 r3 | g3 b3
                const uint32_t d[6] = { s[0][0] | (s[1][0] << 16), s[2][0] | (s[0][1] << 16), s[1][1] | (s[2][1] << 16),
                                        s[0][2] | (s[1][2] << 16), s[2][2] | (s[0][3] << 16), s[1][3] | (s[2][3] << 16) };
                win_store_dwords<6>(q, a.a8 != 0, d);
            } else {
                const uint32_t al = (uint32_t)a.mx << 16;
                const uint32_t d[8] = { s[0][0] | (s[1][0] << 16), s[2][0] | al, s[0][1] | (s[1][1] << 16), s[2][1] | al,
                                        s[0][2] | (s[1][2] << 16), s[2][2] | al, s[0][3] | (s[1][3] << 16), s[2][3] | al };
                win_store_dwords<8>(q, a.a8 != 0, d);
            }
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                if (j < nvis) {
                    uint16_t *const px = reinterpret_cast<uint16_t *>(q) + j * LT::spp;
#pragma unroll
                    for (int k = 0; k < 3; k++) px[k] = (uint16_t)s[k][j];
                    if (LT::spp == 4) px[3] = (uint16_t)a.mx;
                }
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// The decoder's rectangle table of a window plan (BpcArgs::win_n ...); returns the waves of one frame
inline int window_bpc_table(BpcArgs &a, const WindowPlan &p)
{
    static_assert(kWindowMaxRects == kBpcWinRects, "the plan's rectangles fill the decoder's table");
    a.ncx_r = a.ncb_r = 0;
    a.win_n = p.n_rects;
    int before = 0;
    for (int i = 0; i < kBpcWinRects; i++) {
        const bool used = i < p.n_rects;
        a.win_x[i] = used ? p.cb[i].x0 : 0;
        a.win_y[i] = used ? p.cb[i].y0 : 0;
        a.win_w[i] = used ? p.cb[i].x1 - p.cb[i].x0 : 1;
        a.win_before[i] = before;
        if (used) before += (p.cb[i].x1 - p.cb[i].x0) * (p.cb[i].y1 - p.cb[i].y0);
    }
    a.win_before[kBpcWinRects] = before;
    return window_waves(p);
}

// The synthesis launches of a window plan, level wl - 1 first.  Level l > r writes its compact rectangle into `work`
// (one frame's T[P + extra] scratch): levels r + 1, r + 3, ... at element P (each at most P / 4 samples: the `extra`
// region, wl >= 2 whenever such a level exists), levels r + 2, r + 4, ... at element 0; level r (rgb) at element 0.
// Level r of a grey call writes the pixels: u8 != nullptr -- a deep context's (px_max > 0) as uint16 samples clamped to
// px_max, `pitch` in bytes: WinLaunch::out says which form (kWinOutT ...), ::u8 that it is kWinOutU8.
struct WinLaunch { WinSynArgs a; dim3 grid; bool u8; int out; };
inline std::vector<WinLaunch> plan_window_synthesis(const WindowPlan &p, const int32_t *mallat, void *work, size_t P, int aw,
                                                    int ah, float qs, uint8_t *u8, size_t pitch, int off, int px_max = 0)
{
    std::vector<WinLaunch> v;
    for (int l = p.wl - 1; l >= p.r; l--) {
        WinLaunch f;
        WinSynArgs &a = f.a;
        a.mallat = mallat; a.AW = aw;
        a.first = l == p.wl - 1 ? 1 : 0;
        const IRect &in = p.R[l + 1], &out = p.R[l];
        if (a.first) { a.ll = mallat; a.ll_x0 = a.ll_y0 = 0; a.ll_stride = aw; }
        else {
            a.ll = (const char *)work + (((l + 1 - p.r) & 1) ? P : 0) * 4;
            a.ll_x0 = in.x0; a.ll_y0 = in.y0; a.ll_stride = in.x1 - in.x0;
        }
        a.W = aw >> l; a.H = ah >> l;
        a.x0 = out.x0; a.y0 = out.y0; a.x1 = out.x1; a.y1 = out.y1;
        a.dst = (char *)work + (((l - p.r) & 1) ? P : 0) * 4;
        a.dst_u8 = l == p.r ? u8 : nullptr;
        a.pitch = pitch;
        a.off = off;
        a.px_max = px_max;
        a.qs = qs;
        for (int k = 0; k < 4; k++) a.q[k] = kQSteps[l][k];
        a.mallat_z = a.ll_z = a.dst_z = a.u8_z = 0;
        f.grid = dim3((unsigned)((out.x1 - out.x0 + kWinTile - 1) / kWinTile), (unsigned)((out.y1 - out.y0 + kWinTile - 1) / kWinTile), 1);
        f.out = a.dst_u8 == nullptr ? kWinOutT : (px_max > 0 ? kWinOutU16 : kWinOutU8);
        f.u8 = f.out == kWinOutU8;
        v.push_back(f);
    }
    return v;
}

}  // namespace picsong
