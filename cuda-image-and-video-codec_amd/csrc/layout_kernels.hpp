// layout_kernels.hpp -- frames as applications hold them (picsong_ingest_frames, picsong_emit_frames and the whole-frame
// calls over them): W x H pixels at a byte pitch, one byte a pixel or interleaved RGB(A), to and from the codec's padded
// planar u8 planes (AW x AH, row stride AW, plane c of a frame at + c * P).
//
// ingest_kernel<LAYOUT, VEC> pads and de-interleaves in one pass.  The mirror rule is picsong_pad_frame_host's: column
// W + j = column W - 1 - j, padded row H + r = padded row H - 1 - r.
//   A thread makes a GROUP of columns of one row: 16 of a one-byte layout (a dwordx4 in, a dwordx4 out), 4 pixels of
//   an interleaved one (RGBA: a dwordx4 in; RGB24: three dwords; a dword out per plane, repacked with byte permutes).
//   A workgroup takes whole rows: `rows` of them when a row's groups fill only a part of its 256 threads, one row in
//   passes of 256 groups otherwise.  Only source rows 0 .. H - 1 are read, each byte of them once:
//     - the row's last partial group is read per byte, so nothing past row * pitch + W * bpp is touched;
//     - every thread whose columns lie within kLayoutTail of the row's end leaves its bytes in LDS, indexed by their
//       distance j = W - 1 - x from the end; after a barrier the columns from the last whole group on -- the partial
//       group's own and the mirrored ones, at most 19 dwords a row and plane -- are put together from there;
//     - a row that has a mirror image among the padded rows (2 H - 1 - y < AH) is stored twice from the registers.
// emit_kernel<LAYOUT, VEC> is the inverse: crops, interleaves, writes alpha as 255, and writes no byte outside
// [row * pitch, row * pitch + W * bpp) of rows 0 .. H - 1 (the last partial group per byte).
//
// VEC: the image side's pointer, pitch and strides are 4-byte aligned and the padded side's 16-byte aligned -- dword
// and dwordx4 accesses (a16: the image side is 16-byte aligned too, dwordx4 where a group is 16 bytes or more).  Else
// the per-byte form: the same groups, every byte loaded and stored on its own; the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace picsong {

constexpr int kLayoutGrey8 = 0, kLayoutPlanar3 = 1, kLayoutRgb24 = 2, kLayoutBgr24 = 3, kLayoutRgba32 = 4, kLayoutBgra32 = 5;
constexpr int kLayoutCount = 6;             // the layouts of 8-bit contexts
constexpr int kLayoutGrey16 = 6;            // deep contexts' one layout: 2 bytes a pixel (native uint16), the padded side uint16 planes
// deep RGB contexts' layouts (native uint16 samples; the padded side three uint16 planes a frame): three planes
// plane_stride bytes apart; interleaved R, G, B (6 bytes a pixel); interleaved R, G, B, A (8 bytes; A ignored on input,
// written as LayoutArgs::px_max on output)
constexpr int kLayoutPlanar3_16 = 7, kLayoutRgb48 = 8, kLayoutRgba64 = 9;
constexpr int kLayoutMaxFrames = 64;
constexpr int kLayoutTail = 80;             // bytes a row and plane kept for the pad phase: 63 mirrored + 15 of a partial group
constexpr int kLayoutLds = 64 * kLayoutTail;

template <int L> struct LayoutTraits {
    static constexpr bool inter = L >= kLayoutRgb24;                    // interleaved: a thread makes all three planes
    static constexpr int bpp = L < kLayoutRgb24 ? 1 : (L < kLayoutRgba32 ? 3 : 4);
    static constexpr int ppt = inter ? 4 : 16;                           // pixels a thread (a group)
    static constexpr int np = inter ? 3 : 1;                             // planes a thread
    static constexpr int nw = ppt / 4;                                   // dwords a thread and plane
    static constexpr int r = (L == kLayoutBgr24 || L == kLayoutBgra32) ? 2 : 0;   // the byte of R in a pixel (B: 2 - r)
    static constexpr int max_rows = 64 / np;                             // rows a workgroup: kLayoutLds holds their tails
};

struct LayoutArgs {
    uint8_t *img;                           // frame f at img + f * frame_stride, row y at + y * pitch; planar: plane c at + c * plane_stride
    unsigned long long pitch, plane_stride, frame_stride;
    uint8_t *pad;                           // frame f at pad + f * pad_stride, plane c at + c * P, row stride AW
    unsigned long long pad_stride, P;
    int W, H, AW, AH;
    int a16;                                // the image side is 16-byte aligned as well (VEC only)
    int px_max;                             // the 16-bit colour layouts' emit: the alpha sample, 2^(bit depth) - 1; 0 everywhere else
};

// rows of a workgroup: as many as its 256 threads hold groups of, the LDS tails permitting
__host__ __device__ inline uint32_t layout_rows(uint32_t groups, uint32_t max_rows)
{
    const uint32_t r = groups >= 256u ? 1u : 256u / groups;
    return r > max_rows ? max_rows : r;
}

// the byte of plane c (0, 1, 2 = R, G, B) in a pixel
template <int L> __device__ __forceinline__ constexpr int layout_chan(int c)
{
    return !LayoutTraits<L>::inter ? 0 : (c == 1 ? 1 : (c == 0 ? LayoutTraits<L>::r : 2 - LayoutTraits<L>::r));
}

__device__ __forceinline__ uint32_t perm_b32(uint32_t hi, uint32_t lo, uint32_t sel)     // bytes 0-3: lo, 4-7: hi; 0x0C: 0, 0x0D: 0xFF
{
    return __builtin_amdgcn_perm(hi, lo, sel);
}

// ---- the pixels of a whole group, vector form: p[c][k] = dword k of plane c
template <int L>
__device__ __forceinline__ void layout_load_vec(const uint8_t *q, bool a16, uint32_t (&p)[LayoutTraits<L>::np][LayoutTraits<L>::nw])
{
    using T = LayoutTraits<L>;
    if constexpr (!T::inter || T::bpp == 4) {
        uint32_t w[4];
        if (a16) {
            const uint4 x = *reinterpret_cast<const uint4 *>(q);
            w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] = reinterpret_cast<const uint32_t *>(q)[k];
        }
        if constexpr (!T::inter) {
#pragma unroll
            for (int k = 0; k < 4; k++) p[0][k] = w[k];
        } else {
            // four pixels, a dword each: byte b of all four
#pragma unroll
            for (int c = 0; c < T::np; c++) {
                const uint32_t b = (uint32_t)layout_chan<L>(c), sel = 0x0C0C0000u | ((4u + b) << 8) | b;
                p[c][0] = perm_b32(perm_b32(w[3], w[2], sel), perm_b32(w[1], w[0], sel), 0x05040100u);
            }
        }
    } else {
        // four pixels in three dwords, x g z the pixel's bytes 0 1 2: x0 g0 z0 x1 | g1 z1 x2 g2 | z2 x3 g3 z3
        const uint32_t d0 = reinterpret_cast<const uint32_t *>(q)[0], d1 = reinterpret_cast<const uint32_t *>(q)[1],
                       d2 = reinterpret_cast<const uint32_t *>(q)[2];
        p[T::r][0] = perm_b32(d2, perm_b32(d1, d0, 0x0C060300u), 0x05020100u);
        p[1][0] = perm_b32(d2, perm_b32(d1, d0, 0x0C070401u), 0x06020100u);
        p[2 - T::r][0] = perm_b32(d2, perm_b32(d1, d0, 0x0C0C0502u), 0x07040100u);
    }
}

// ---- the first nvis pixels of a group, per byte (the other bytes: 0)
template <int L>
__device__ __forceinline__ void layout_load_bytes(const uint8_t *q, uint32_t nvis, uint32_t (&p)[LayoutTraits<L>::np][LayoutTraits<L>::nw])
{
    using T = LayoutTraits<L>;
#pragma unroll
    for (int c = 0; c < T::np; c++)
#pragma unroll
        for (int k = 0; k < T::nw; k++) p[c][k] = 0u;
#pragma unroll
    for (int i = 0; i < T::ppt; i++) {
        if ((uint32_t)i < nvis) {
#pragma unroll
            for (int c = 0; c < T::np; c++) p[c][i / 4] |= (uint32_t)q[i * T::bpp + layout_chan<L>(c)] << (8 * (i % 4));
        }
    }
}

// NW dwords to a padded plane
template <bool VEC, int NW>
__device__ __forceinline__ void layout_store_plane(uint8_t *d, const uint32_t (&w)[NW])
{
    if constexpr (VEC) {
        if constexpr (NW == 4) {
            uint4 x;
            x.x = w[0]; x.y = w[1]; x.z = w[2]; x.w = w[3];
            *reinterpret_cast<uint4 *>(d) = x;
        } else {
#pragma unroll
            for (int k = 0; k < NW; k++) reinterpret_cast<uint32_t *>(d)[k] = w[k];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4 * NW; i++) d[i] = (uint8_t)(w[i / 4] >> (8 * (i % 4)));
    }
}

template <int L, bool VEC>
__global__ __launch_bounds__(256) void ingest_kernel(LayoutArgs s)
{
    using T = LayoutTraits<L>;
    constexpr uint32_t PPT = T::ppt, NP = T::np;
    __shared__ uint8_t tail[kLayoutLds];    // [row of the workgroup][plane][distance from the row's end]
    const uint32_t W = (uint32_t)s.W, H = (uint32_t)s.H, AW = (uint32_t)s.AW, AH = (uint32_t)s.AH;
    const uint32_t gv = (W + PPT - 1u) / PPT;                            // groups with a visible column
    const uint32_t rows = layout_rows(gv, (uint32_t)T::max_rows);
    const uint32_t tid = threadIdx.x, r = rows == 1u ? 0u : tid / gv, g0 = tid - r * gv;
    const uint32_t row0 = blockIdx.x * rows, y = row0 + r;
    const uint32_t ym = 2u * H - 1u - y;                                 // the padded row that mirrors row y, if < AH
    uint8_t *const dst = s.pad + (size_t)blockIdx.z * s.pad_stride + (size_t)blockIdx.y * s.P;

    if (r < rows && y < H) {
        const uint8_t *const src = s.img + (size_t)blockIdx.z * s.frame_stride + (size_t)blockIdx.y * s.plane_stride + (size_t)y * s.pitch;
        for (uint32_t g = g0; g < gv; g += 256u) {
            const uint32_t x0 = g * PPT, nvis = W - x0 < PPT ? W - x0 : PPT;
            uint32_t p[T::np][T::nw];
            if (VEC && nvis == PPT) layout_load_vec<L>(src + (size_t)x0 * T::bpp, s.a16 != 0, p);
            else layout_load_bytes<L>(src + (size_t)x0 * T::bpp, nvis, p);
            if (nvis == PPT) {
#pragma unroll
                for (uint32_t c = 0; c < NP; c++) {
                    layout_store_plane<VEC>(dst + (size_t)c * s.P + (size_t)y * AW + x0, p[c]);
                    if (ym < AH) layout_store_plane<VEC>(dst + (size_t)c * s.P + (size_t)ym * AW + x0, p[c]);
                }
            }
            if (x0 + PPT + (uint32_t)kLayoutTail > W) {
#pragma unroll
                for (uint32_t i = 0; i < PPT; i++) {
                    const uint32_t j = W - 1u - (x0 + i);                // (wraps to a huge value for the bytes past the row's end)
                    if (i < nvis && j < (uint32_t)kLayoutTail) {
#pragma unroll
                        for (uint32_t c = 0; c < NP; c++) tail[(r * NP + c) * (uint32_t)kLayoutTail + j] = (uint8_t)(p[c][i / 4u] >> (8u * (i % 4u)));
                    }
                }
            }
        }
    }
    __syncthreads();
    // ---- the columns from the last whole group on: the partial group's own bytes and the mirrored ones, a dword an item
    const uint32_t xe = (W / PPT) * PPT, nq = (AW - xe) / 4u;
    const uint32_t rows_here = H - row0 < rows ? H - row0 : rows;
    for (uint32_t t = tid; t < rows_here * NP * nq; t += 256u) {
        const uint32_t q = t % nq, rc = t / nq, c = rc % NP, rr = rc / NP;
        const uint32_t yy = row0 + rr, yym = 2u * H - 1u - yy;
        uint32_t w[1] = { 0u };
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {
            const uint32_t x = xe + 4u * q + i, j = x < W ? W - 1u - x : x - W;
            w[0] |= (uint32_t)tail[(rr * NP + c) * (uint32_t)kLayoutTail + j] << (8u * i);
        }
        layout_store_plane<VEC>(dst + (size_t)c * s.P + (size_t)yy * AW + xe + 4u * q, w);
        if (yym < AH) layout_store_plane<VEC>(dst + (size_t)c * s.P + (size_t)yym * AW + xe + 4u * q, w);
    }
}

// ---- a whole group of pixels to the image, vector form
template <int L>
__device__ __forceinline__ void layout_store_vec(uint8_t *q, bool a16, const uint32_t (&p)[LayoutTraits<L>::np][LayoutTraits<L>::nw])
{
    using T = LayoutTraits<L>;
    uint32_t w[4];
    if constexpr (!T::inter) {
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = p[0][k];
    } else {
        const uint32_t x = p[T::r][0], g = p[1][0], z = p[2 - T::r][0];                                     // the pixel's bytes 0, 1, 2
        if constexpr (T::bpp == 4) {
            const uint32_t xg_lo = perm_b32(g, x, 0x05010400u), xg_hi = perm_b32(g, x, 0x07030602u);
            const uint32_t za_lo = perm_b32(0u, z, 0x0D010D00u), za_hi = perm_b32(0u, z, 0x0D030D02u);      // alpha: 255
            w[0] = perm_b32(za_lo, xg_lo, 0x05040100u); w[1] = perm_b32(za_lo, xg_lo, 0x07060302u);
            w[2] = perm_b32(za_hi, xg_hi, 0x05040100u); w[3] = perm_b32(za_hi, xg_hi, 0x07060302u);
        } else {
            // x0 g0 z0 x1 | g1 z1 x2 g2 | z2 x3 g3 z3
            reinterpret_cast<uint32_t *>(q)[0] = perm_b32(z, perm_b32(g, x, 0x010C0400u), 0x03040100u);
            reinterpret_cast<uint32_t *>(q)[1] = perm_b32(z, perm_b32(g, x, 0x06020C05u), 0x03020500u);
            reinterpret_cast<uint32_t *>(q)[2] = perm_b32(z, perm_b32(g, x, 0x0C07030Cu), 0x07020106u);
            return;
        }
    }
    if (a16) {
        uint4 v;
        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
        *reinterpret_cast<uint4 *>(q) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) reinterpret_cast<uint32_t *>(q)[k] = w[k];
    }
}

template <int L, bool VEC>
__global__ __launch_bounds__(256) void emit_kernel(LayoutArgs s)
{
    using T = LayoutTraits<L>;
    constexpr uint32_t PPT = T::ppt, NP = T::np;
    const uint32_t W = (uint32_t)s.W, H = (uint32_t)s.H, AW = (uint32_t)s.AW;
    const uint32_t gv = (W + PPT - 1u) / PPT;
    const uint32_t rows = layout_rows(gv, (uint32_t)T::max_rows);
    const uint32_t tid = threadIdx.x, r = rows == 1u ? 0u : tid / gv, g0 = tid - r * gv;
    const uint32_t y = blockIdx.x * rows + r;
    if (r >= rows || y >= H) return;
    const uint8_t *const src = s.pad + (size_t)blockIdx.z * s.pad_stride + (size_t)blockIdx.y * s.P + (size_t)y * AW;
    uint8_t *const dst = s.img + (size_t)blockIdx.z * s.frame_stride + (size_t)blockIdx.y * s.plane_stride + (size_t)y * s.pitch;
    for (uint32_t g = g0; g < gv; g += 256u) {
        const uint32_t x0 = g * PPT, nvis = W - x0 < PPT ? W - x0 : PPT;
        uint32_t p[T::np][T::nw];
        // (a whole group of the padded row is always there: AW is a multiple of 64)
#pragma unroll
        for (uint32_t c = 0; c < NP; c++) {
            const uint8_t *const pc = src + (size_t)c * s.P + x0;
            if constexpr (VEC) {
                if constexpr (T::nw == 4) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(pc);
                    p[c][0] = v.x; p[c][1] = v.y; p[c][2] = v.z; p[c][3] = v.w;
                } else {
                    p[c][0] = *reinterpret_cast<const uint32_t *>(pc);
                }
            } else {
#pragma unroll
                for (int k = 0; k < T::nw; k++)
                    p[c][k] = (uint32_t)pc[4 * k] | ((uint32_t)pc[4 * k + 1] << 8) | ((uint32_t)pc[4 * k + 2] << 16) | ((uint32_t)pc[4 * k + 3] << 24);
            }
        }
        uint8_t *const q = dst + (size_t)x0 * T::bpp;
        if (VEC && nvis == PPT) {
            layout_store_vec<L>(q, s.a16 != 0, p);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < PPT; i++) {
                if (i < nvis) {
#pragma unroll
                    for (uint32_t c = 0; c < NP; c++) q[i * T::bpp + layout_chan<L>((int)c)] = (uint8_t)(p[c][i / 4u] >> (8u * (i % 4u)));
                    if (T::bpp == 4) q[i * T::bpp + 3u] = 0xFFu;
                }
            }
        }
    }
}

// ---- GREY16 (deep contexts): W x H native uint16 samples at a byte pitch, to and from a padded uint16 plane (row stride
// AW samples; frame f at pad + f * pad_stride BYTES).  The mirror rule is picsong_pad_frame16_host's.
// ingest16_kernel: a thread makes a group of 8 samples (16 bytes) of one PADDED row, from the source row that row
// mirrors; only bytes [y * pitch, y * pitch + 2 W) of the source rows 0 .. H - 1 are read.  emit16_kernel crops: a thread
// a group of 8 samples of a visible row, and no byte outside [y * pitch, y * pitch + 2 W) of rows 0 .. H - 1 is written.
// VEC: the padded side 16-byte, the image side 4-byte aligned -- a dwordx4 on the padded side, dwords on the image side for a
// group that lies wholly inside the row.  Else every sample on its own; the same bytes.
template <bool VEC>
__global__ __launch_bounds__(256) void ingest16_kernel(LayoutArgs s)
{
    const uint32_t W = (uint32_t)s.W, H = (uint32_t)s.H, AW = (uint32_t)s.AW, AH = (uint32_t)s.AH;
    const uint32_t gpr = AW / 8u;
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (size_t)gpr * AH) return;
    const uint32_t y = (uint32_t)(t / gpr), x0 = (uint32_t)(t % gpr) * 8u;
    const uint32_t sy = y < H ? y : 2u * H - 1u - y;
    const uint8_t *const src = s.img + (size_t)blockIdx.z * s.frame_stride + (size_t)sy * s.pitch;
    uint8_t *const dst = s.pad + (size_t)blockIdx.z * s.pad_stride + ((size_t)y * AW + x0) * 2u;
    uint32_t w[4];
    if (VEC && x0 + 8u <= W) {
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = reinterpret_cast<const uint32_t *>(src + (size_t)x0 * 2u)[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t xa = x0 + 2u * k, xb = xa + 1u;
            const uint32_t sa = xa < W ? xa : 2u * W - 1u - xa, sb = xb < W ? xb : 2u * W - 1u - xb;
            w[k] = (uint32_t)reinterpret_cast<const uint16_t *>(src)[sa] | ((uint32_t)reinterpret_cast<const uint16_t *>(src)[sb] << 16);
        }
    }
    if constexpr (VEC) {
        uint4 v;
        v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
        *reinterpret_cast<uint4 *>(dst) = v;
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) reinterpret_cast<uint16_t *>(dst)[i] = (uint16_t)(w[i / 2] >> (16 * (i % 2)));
    }
}
template <bool VEC>
__global__ __launch_bounds__(256) void emit16_kernel(LayoutArgs s)
{
    const uint32_t W = (uint32_t)s.W, H = (uint32_t)s.H, AW = (uint32_t)s.AW;
    const uint32_t gpr = (W + 7u) / 8u;
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (size_t)gpr * H) return;
    const uint32_t y = (uint32_t)(t / gpr), x0 = (uint32_t)(t % gpr) * 8u;
    const uint32_t nvis = W - x0 < 8u ? W - x0 : 8u;
    // (a whole group of the padded row is always there: AW is a multiple of 64)
    const uint8_t *const src = s.pad + (size_t)blockIdx.z * s.pad_stride + ((size_t)y * AW + x0) * 2u;
    uint8_t *const dst = s.img + (size_t)blockIdx.z * s.frame_stride + (size_t)y * s.pitch + (size_t)x0 * 2u;
    uint32_t w[4];
    if constexpr (VEC) {
        const uint4 v = *reinterpret_cast<const uint4 *>(src);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            w[k] = (uint32_t)reinterpret_cast<const uint16_t *>(src)[2 * k] | ((uint32_t)reinterpret_cast<const uint16_t *>(src)[2 * k + 1] << 16);
    }
    if (VEC && nvis == 8u) {
#pragma unroll
        for (int k = 0; k < 4; k++) reinterpret_cast<uint32_t *>(dst)[k] = w[k];
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++)
            if (i < nvis) reinterpret_cast<uint16_t *>(dst)[i] = (uint16_t)(w[i / 2u] >> (16u * (i % 2u)));
    }
}

// ---- the 16-bit colour layouts (deep RGB contexts): kLayoutPlanar3_16, kLayoutRgb48, kLayoutRgba64 to and from three padded
// uint16 planes a frame (plane c of frame f at pad + f * pad_stride + c * 2 P BYTES, row stride AW samples).  The scheme is
// ingest16_kernel's / emit16_kernel's: ingest_rgb16_kernel runs over the PADDED rows, a thread a group of 8 pixels of one,
// reads the source row that row mirrors -- only bytes [y * pitch, y * pitch + W * bpp) of rows 0 .. H - 1 -- and
// de-interleaves in the same pass; emit_rgb16_kernel crops and interleaves, a thread 8 pixels of a visible row, alpha = px_max,
// and writes no byte outside [y * pitch, y * pitch + W * bpp).  The planar layout runs a plane a grid.y.
// VEC: a dwordx4 a plane on the padded side (16-byte aligned); dwords on the image side where it is 4-byte aligned and the
// group lies wholly inside the row.  Else every sample on its own; the same bytes.
template <int L> struct Layout16Traits {
    static constexpr int spp = L == kLayoutRgb48 ? 3 : (L == kLayoutRgba64 ? 4 : 1);     // samples a pixel on the image side
    static constexpr int np = L == kLayoutPlanar3_16 ? 1 : 3;                            // planes a thread
};
__device__ __forceinline__ uint32_t half_of(const uint32_t *w, int h) { return (w[h >> 1] >> (16 * (h & 1))) & 0xFFFFu; }

template <int L, bool VEC>
__global__ __launch_bounds__(256) void ingest_rgb16_kernel(LayoutArgs s)
{
    using T = Layout16Traits<L>;
    const uint32_t W = (uint32_t)s.W, H = (uint32_t)s.H, AW = (uint32_t)s.AW, AH = (uint32_t)s.AH;
    const uint32_t gpr = AW / 8u;
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (size_t)gpr * AH) return;
    const uint32_t y = (uint32_t)(t / gpr), x0 = (uint32_t)(t % gpr) * 8u;
    const uint32_t sy = y < H ? y : 2u * H - 1u - y;
    const uint8_t *const src = s.img + (size_t)blockIdx.z * s.frame_stride + (size_t)blockIdx.y * s.plane_stride + (size_t)sy * s.pitch;
    uint8_t *const dst = s.pad + (size_t)blockIdx.z * s.pad_stride + (size_t)blockIdx.y * s.P * 2u + ((size_t)y * AW + x0) * 2u;
    uint32_t p[T::np][4];
#pragma unroll
    for (int c = 0; c < T::np; c++)
#pragma unroll
        for (int k = 0; k < 4; k++) p[c][k] = 0u;
    if (VEC && x0 + 8u <= W) {
        uint32_t w[4 * T::spp];
#pragma unroll
        for (int k = 0; k < 4 * T::spp; k++) w[k] = reinterpret_cast<const uint32_t *>(src + (size_t)x0 * 2u * T::spp)[k];
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int c = 0; c < T::np; c++) p[c][i >> 1] |= half_of(w, T::spp * i + c) << (16 * (i & 1));
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++) {
            const uint32_t x = x0 + i, sx = x < W ? x : 2u * W - 1u - x;
#pragma unroll
            for (int c = 0; c < T::np; c++)
                p[c][i >> 1] |= (uint32_t)reinterpret_cast<const uint16_t *>(src)[(size_t)sx * T::spp + c] << (16u * (i & 1u));
        }
    }
#pragma unroll
    for (int c = 0; c < T::np; c++) {
        uint8_t *const d = dst + (size_t)c * s.P * 2u;
        if constexpr (VEC) {
            uint4 v;
            v.x = p[c][0]; v.y = p[c][1]; v.z = p[c][2]; v.w = p[c][3];
            *reinterpret_cast<uint4 *>(d) = v;
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) reinterpret_cast<uint16_t *>(d)[i] = (uint16_t)half_of(p[c], i);
        }
    }
}

template <int L, bool VEC>
__global__ __launch_bounds__(256) void emit_rgb16_kernel(LayoutArgs s)
{
    using T = Layout16Traits<L>;
    const uint32_t W = (uint32_t)s.W, H = (uint32_t)s.H, AW = (uint32_t)s.AW;
    const uint32_t gpr = (W + 7u) / 8u;
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (size_t)gpr * H) return;
    const uint32_t y = (uint32_t)(t / gpr), x0 = (uint32_t)(t % gpr) * 8u;
    const uint32_t nvis = W - x0 < 8u ? W - x0 : 8u;
    // (a whole group of the padded row is always there: AW is a multiple of 64)
    const uint8_t *const src = s.pad + (size_t)blockIdx.z * s.pad_stride + (size_t)blockIdx.y * s.P * 2u + ((size_t)y * AW + x0) * 2u;
    uint8_t *const dst = s.img + (size_t)blockIdx.z * s.frame_stride + (size_t)blockIdx.y * s.plane_stride + (size_t)y * s.pitch +
                         (size_t)x0 * 2u * T::spp;
    uint32_t p[T::np][4];
#pragma unroll
    for (int c = 0; c < T::np; c++) {
        const uint8_t *const q = src + (size_t)c * s.P * 2u;
        if constexpr (VEC) {
            const uint4 v = *reinterpret_cast<const uint4 *>(q);
            p[c][0] = v.x; p[c][1] = v.y; p[c][2] = v.z; p[c][3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                p[c][k] = (uint32_t)reinterpret_cast<const uint16_t *>(q)[2 * k] | ((uint32_t)reinterpret_cast<const uint16_t *>(q)[2 * k + 1] << 16);
        }
    }
    const uint32_t alpha = (uint32_t)s.px_max & 0xFFFFu;
    if (VEC && nvis == 8u) {
        uint32_t w[4 * T::spp];
#pragma unroll
        for (int k = 0; k < 4 * T::spp; k++) w[k] = 0u;
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int c = 0; c < T::spp; c++) {
                const int h = T::spp * i + c;
                w[h >> 1] |= (c < T::np ? half_of(p[c < T::np ? c : 0], i) : alpha) << (16 * (h & 1));
            }
#pragma unroll
        for (int k = 0; k < 4 * T::spp; k++) reinterpret_cast<uint32_t *>(dst)[k] = w[k];
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++)
            if (i < nvis) {
#pragma unroll
                for (int c = 0; c < T::spp; c++)
                    reinterpret_cast<uint16_t *>(dst)[i * T::spp + c] = (uint16_t)(c < T::np ? half_of(p[c < T::np ? c : 0], (int)i) : alpha);
            }
    }
}

}  // namespace picsong
