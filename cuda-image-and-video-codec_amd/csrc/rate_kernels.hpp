// rate_kernels.hpp -- the quantisation pass of the rate calls (picsong_encode_frame_rate and its mirrors).
//
// The 9/7 forward transform fuses its quantisation into the last step of every level: a coefficient leaves as
// (T)(((float)x * q[level][subband]) * qs) (emit_pair and the fused head, dwt_kernels.hpp).  With every step and qs at
// 1.0f the transform is exact (x * 1.0f * 1.0f is x), so the coefficients of ANY qs follow from the unquantised Mallat
// array by one element-wise pass with those two multiplications in that order: the fused path's bits.
//
// quantise_kernel reads the unquantised float arrays of n frames once and writes, for each of K candidate gains, the
// array the coder takes: int16 through pack_c16's conversion (toward zero, as the coder's own load of a float) or the
// float product itself, per candidate.  Candidate c of frame f lands at dst + (c * n + f) * dst_z: "frame" c * n + f of a
// batched coder launch.
// I32 (the quality calls' probes, picsong_encode_frame_quality): every candidate leaves as an int32 Mallat array, the
// float product truncated toward zero -- what the coder codes and the decoder returns, the form the synthesis reads.
//
// A bandwidth-bound stream: 256 threads, 16 bytes a lane and load, a workgroup a row at a time (grid-stride over the
// n * AH rows), so a wave's row and with it the vertical half of the subband search is uniform.  Subband edges are not
// vector-aligned in general (AW = 704, wl = 6: an edge at column 11), so every element of a group of four takes its own
// step -- from vector registers: a multiply with a scalar-register operand issues at half rate.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dwt_kernels.hpp"

namespace picsong {

constexpr int kQuantMaxK = 3;

struct QuantArgs {
    const void *src;                // n float Mallat arrays (row stride AW), src_z bytes apart
    unsigned long long src_z;
    void *dst;                      // candidate c of frame f: dst + (c * n + f) * dst_z bytes, int16, float or int32 [AH x AW]
    unsigned long long dst_z;
    int AW, AH, wl, n;
    int c16[kQuantMaxK];            // candidate c leaves as int16 (else float)
    float qs[kQuantMaxK];
    float q[10][4];                 // kQSteps: row = level, columns LL, HL, LH, HH
};

// The step of the element at column x of a row whose vertical level is ly (the smallest l with y >= AH >> (l + 1), wl
// when there is none).  With lx the same for x and AW: lx < ly -> HL of level lx; lx == ly < wl -> HH; lx > ly -> LH of
// level ly; both wl -> LL, which takes row wl - 1, column 0.  rs[l]: the step of the columns [AW >> (l + 1), AW >> l) of
// this row; low: that of the columns below AW >> wl.
template <int K, bool I32 = false>
__global__ __launch_bounds__(256) void quantise_kernel(QuantArgs a)
{
    static_assert(K >= 1 && K <= kQuantMaxK, "one to three candidates a launch");
    const uint32_t groups = (uint32_t)a.AW >> 2, rows = (uint32_t)a.n * (uint32_t)a.AH;
    float vqs[K];
#pragma unroll
    for (int c = 0; c < K; c++) vqs[c] = in_vgpr(a.qs[c]);
    for (uint32_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const uint32_t f = r / (uint32_t)a.AH, y = r - f * (uint32_t)a.AH;      // (workgroup-uniform)
        int ly = a.wl;
        for (int l = a.wl - 1; l >= 0; l--) if (y >= (uint32_t)(a.AH >> (l + 1))) ly = l;
        // (the row's steps as vector registers; the levels' own entries are read with constant indices)
        float low_s = a.q[0][0];
#pragma unroll
        for (int l = 0; l < 10; l++) {
            if (l == ly && ly < a.wl) low_s = a.q[l][2];
            if (ly == a.wl && l == a.wl - 1) low_s = a.q[l][0];
        }
        const float low = in_vgpr(low_s);
        float rs[10];
#pragma unroll
        for (int l = 0; l < 10; l++) rs[l] = in_vgpr(l < ly ? a.q[l][1] : (l == ly ? a.q[l][3] : low_s));
        const float4 *const srow = reinterpret_cast<const float4 *>((const char *)a.src + (unsigned long long)f * a.src_z) +
                                   (size_t)y * groups;
        for (uint32_t g = threadIdx.x; g < groups; g += 256u) {
            const float4 v = srow[g];
            const float x[4] = { v.x, v.y, v.z, v.w };
            float st[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const uint32_t col = 4u * g + (uint32_t)e;
                float s = low;
#pragma unroll
                for (int l = 9; l >= 0; l--)
                    if (l < a.wl) s = col >= (uint32_t)(a.AW >> (l + 1)) ? rs[l] : s;
                st[e] = s;
            }
#pragma unroll
            for (int c = 0; c < K; c++) {
                float t[4];
#pragma unroll
                for (int e = 0; e < 4; e++) t[e] = (x[e] * st[e]) * vqs[c];     // emit_pair's operations, in its order
                char *const base = (char *)a.dst + (unsigned long long)((uint32_t)c * (uint32_t)a.n + f) * a.dst_z;
                if (I32) {
                    uint4 w;
                    w.x = (uint32_t)(int)t[0]; w.y = (uint32_t)(int)t[1]; w.z = (uint32_t)(int)t[2]; w.w = (uint32_t)(int)t[3];
                    reinterpret_cast<uint4 *>(base)[(size_t)y * groups + g] = w;
                } else if (a.c16[c]) {
                    uint2 w;
                    w.x = pack_c16(t[0], t[1]); w.y = pack_c16(t[2], t[3]);
                    reinterpret_cast<uint2 *>(base)[(size_t)y * groups + g] = w;
                } else {
                    reinterpret_cast<float4 *>(base)[(size_t)y * groups + g] = make_float4(t[0], t[1], t[2], t[3]);
                }
            }
        }
    }
}

}  // namespace picsong
