// picsong_hip.hip -- C-ABI implementation (include/picsong_hip.h): host launch logic for the
// gfx950 kernels in dwt_kernels.hpp / bpc_kernels.hpp / pack_kernels.hpp / window_kernels.hpp.  Which instantiation a
// launch takes, its grid and its scratch (kernel_select.hpp) and the launch sequences themselves (launch_seq.hpp) are
// shared with the emulator drivers of tests/hipemu/; here: argument checks, allocation, bookkeeping and the launcher.
// No CPU fallback exists: without a GPU every device entry point returns PICSONG_ERR_NODEVICE.
#include "../../include/picsong_hip.h"

#include <hip/hip_runtime.h>

#include <sys/stat.h>

#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "launch_seq.hpp"

using namespace picsong;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(PICSONG_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                               \
    } while (0)

// The library's launcher (launch_seq.hpp): kernel k over grid x threads on the stream it holds
struct HipGo {
    hipStream_t s;
    template <typename... P, typename... A>
    int operator()(void (*k)(P...), dim3 grid, unsigned threads, const A &...args) const
    {
        k<<<grid, threads, 0, s>>>(args...);
        HIP_TRY(hipGetLastError());
        return PICSONG_OK;
    }
};

}  // namespace

struct picsong_ctx {
    picsong_params p;
    int device;
    int aw, ah, ncb;
    int dec_waves;        // waves of a frame's coder launch the plane scratch holds (dec_scratch_waves)
    size_t P, extra;
    bool fast_div;        // 9/7 synthesis: reciprocal form of the divisions verified for this qs
    bool c16;             // frame paths: coded coefficients travel as int16 between transform and coder (coef16_ok)
    bool c16_dec;         // decode frame paths: ... and between decoder and synthesis (dec_c16_ok)
    int bulk_compact[3];  // -k > 0: the component's table geometry lets every codeblock use the compact LDS copy (-1: not looked at yet)
    bool pipelined;       // picsong_ctx_set_pipelined: other frames share the GPU (throughput over latency)
    int drop;             // picsong_ctx_set_decode_drop: the decoders' BpcArgs::drop (0: every plane)
    // LUT
    picsong_lut_info li[3];
    int32_t *d_lut[3];
    bool has_lut[3];
    bool lut_borrowed[3]; // d_lut[k] is the caller's device table (picsong_ctx_set_lut_device): not freed here
    PlaneRec *d_img[3];   // k = 0, -cp 2: the table's plane records for the encoder (plane_record), kPlaneImgMaxRecs
    int *d_flag;          // 1
    int32_t *h_pinned;    // [0] total, [1] flag
    Workspace one;        // a frame's (lazy: ensure_workspace, ensure_plane_scratch; offsets and total at creation)
    // batched frame path (picsong_encode_frames): workspaces for batch_cap frames, laid frame after frame
    Workspace batch;      // (coef_i: the decoded coefficients of a batch, picsong_decode_frames; b_coef_i_cap planes, lazy)
    int batch_cap, b_coef_i_cap;
    int32_t *h_totals;    // pinned, batch_cap
    int last_batch;       // frames of the most recent picsong_encode_frames
    // stage profiling (HIP events on the launch stream)
    std::vector<hipEvent_t> *prof_ev;   // 4 per frame
    int prof_cap, prof_n;
    // training (picsong_train_begin): the geometry counted for, uint64[train_total][2] per component slot, and the plane
    // scratch of the statistics kernel's persistent grid (grown to the largest launch seen)
    bool train_on;
    picsong_lut_info train_li;
    int train_total;
    unsigned long long *d_train[3];
    uint32_t *train_scratch;
    size_t train_scratch_dwords;
    // rate calls (picsong_encode_frame_rate): the unquantised transform's work buffers, rate_cap frames of rate_z bytes
    void *rate_coef;
    int rate_cap;
    size_t rate_z;
    // quality calls: the probes' clamped pixels (q_cap planes of P bytes), the candidates' sums on the device and pinned
    uint8_t *q_pix;
    int q_cap;
    unsigned long long *d_sse, *h_sse;      // kQualitySlots each (lazy)
    // image calls (picsong_encode_images and its mirrors): the padded planes between the layout kernels and the frame sequences
    uint8_t *lay_buf;
    size_t lay_cap;                         // bytes
};

// PICSONG_DWT_INV97=0 keeps the 9/7 synthesis levels off the lean kernel (select_inv): read once per process
static bool lean97_levels()
{
    static const bool lean97 = !(getenv("PICSONG_DWT_INV97") && atoi(getenv("PICSONG_DWT_INV97")) == 0);
    return lean97;
}

static int level_off(const picsong_ctx *c) { return 1 << (c->p.bit_depth - 1); }
// a deep context: 9- to 16-bit samples, uint16 frames through the *16 calls; its largest sample
static bool is_deep(const picsong_ctx *c) { return c->p.bit_depth > 8; }
static int px_max(const picsong_ctx *c) { return (1 << c->p.bit_depth) - 1; }
// a deep RGB context: three uint16 planes a frame through the *16 RGB calls
static bool is_deep_rgb(const picsong_ctx *c) { return is_deep(c) && c->p.is_rgb != 0; }
// the calls that take or return uint8_t frames, on a deep context (nothing launched)
#define REFUSE_DEEP(c, who)                                                                                              \
    do {                                                                                                                 \
        if ((c) && is_deep_rgb(c))                                                                                       \
            return fail(PICSONG_ERR_ARG, "%s: 8-bit frames on a %d-bit RGB context (its frame calls: "                    \
                                         "picsong_encode_rgb_frames16, picsong_decode_rgb_frames16)", who, (c)->p.bit_depth); \
        if ((c) && is_deep(c))                                                                                           \
            return fail(PICSONG_ERR_ARG, "%s: 8-bit frames on a %d-bit context (its frame calls: picsong_encode_frames16, " \
                                         "picsong_decode_frames16, GREY16 images)", who, (c)->p.bit_depth);             \
    } while (0)
// ... and the uint16 calls on an 8-bit one
#define REFUSE_SHALLOW(c, who)                                                                                           \
    do {                                                                                                                 \
        if ((c) && !is_deep(c)) return fail(PICSONG_ERR_ARG, "%s: uint16 samples on an 8-bit context", who);             \
    } while (0)

extern "C" {

const char *picsong_last_error(void) { return g_err; }
const char *picsong_version(void) { return "picsong-mi355x 0.1 (gfx950)"; }

int picsong_pad_dim(int v) { return ((v + PICSONG_CB - 1) / PICSONG_CB) * PICSONG_CB; }

size_t picsong_dwt_extra(int aw, int ah, int wl)
{
    return dwt_extra(aw, ah, wl);
}

size_t picsong_max_stream_shorts(int aw, int ah)
{
    size_t ncb = (size_t)(aw / PICSONG_CB) * (size_t)(ah / PICSONG_CB);
    return PICSONG_HDR_SHORTS + 2 * ncb + (size_t)aw * (size_t)ah + 1;
}

// ---------------------------------------------------------------------------------------------
// header
// ---------------------------------------------------------------------------------------------
int picsong_header_pack(const picsong_params *p, uint16_t o[PICSONG_HDR_SHORTS])
{
    if (!p || !o) return fail(PICSONG_ERR_ARG, "header_pack: null argument");
    if (p->width <= 0 || p->height <= 0 || p->height > 65535 || p->components <= 0 || p->frames < 0 ||
        p->frames >= (1 << 17) ||
        (uint64_t)p->width * (uint64_t)p->height * (uint64_t)p->components >= ((uint64_t)1 << 32))
        return fail(PICSONG_ERR_ARG, "header_pack: a field exceeds its width (height 16 bits, frames 17, samples 32)");
    const uint32_t n = (uint32_t)p->width * (uint32_t)p->height * (uint32_t)p->components;
    const int qs4 = (int)(p->qs * 10000), k3 = (int)(p->k * 1000);
    o[0] = (uint16_t)(n & 0xFFFFu);
    o[1] = (uint16_t)(n >> 16);
    o[2] = (uint16_t)((p->cp == 2 ? 0 : 1) | (p->cb_height << 1) | (p->cb_width << 8) | ((p->wl & 1) << 15));
    o[3] = (uint16_t)(((p->wl & 7) >> 1) | (p->bit_depth << 3) | ((p->lossy ? 1 : 0) << 10) | ((qs4 & 31) << 11));
    o[4] = (uint16_t)((qs4 >> 5) | ((p->components & 127) << 9));
    o[5] = (uint16_t)((p->components >> 7) | ((p->is_rgb ? 1 : 0) << 7) | (p->height << 8));
    o[6] = (uint16_t)((p->height >> 8) | (0 << 8) | (p->bit_depth << 9) | (0 << 14) | ((p->frames & 1) << 15));
    o[7] = (uint16_t)((p->frames >> 1) & 0xFFFF);
    o[8] = (uint16_t)k3;
    return PICSONG_OK;
}

int picsong_header_unpack(const uint16_t e[PICSONG_HDR_SHORTS], picsong_params *p)
{
    if (!p || !e) return fail(PICSONG_ERR_ARG, "header_unpack: null argument");
    memset(p, 0, sizeof *p);
    const uint32_t n = (uint32_t)e[0] | ((uint32_t)e[1] << 16);
    p->cp = (e[2] & 1) ? 3 : 2;
    p->cb_height = (e[2] >> 1) & 127;
    p->cb_width = (e[2] >> 8) & 127;
    p->wl = ((e[2] >> 15) & 1) | ((e[3] & 7) << 1);
    p->bit_depth = (e[3] >> 3) & 127;
    p->lossy = (e[3] >> 10) & 1;
    p->qs = (float)((((e[3] >> 11) & 31) | ((e[4] & 511) << 5)) / 10000.0);   // DecodingEngine.cu:161
    p->components = ((e[4] >> 9) & 127) | ((e[5] & 127) << 9);
    p->is_rgb = (e[5] >> 7) & 1;
    p->height = ((e[5] >> 8) & 255) | ((e[6] & 255) << 8);
    p->frames = ((e[6] >> 15) & 1) | ((int)e[7] << 1);
    p->k = (float)(e[8] / 1000.0);
    if (p->height <= 0 || p->components <= 0) return fail(PICSONG_ERR_ARG, "header_unpack: bad header");
    p->width = (int)(n / (uint32_t)p->height / (uint32_t)p->components);       // DecodingEngine.cu:146
    return PICSONG_OK;
}

// ---------------------------------------------------------------------------------------------
// LUT text parser
// ---------------------------------------------------------------------------------------------
static int lut_section(const std::string &folder, const char *stem, int component, int file_index, int C, int nBp,
                       int wl, int32_t *T, int base, size_t cap)
{
    static const char *suffix[4] = { ".txt_", "R.txt_", "G.txt_", "B.txt_" };
    std::string path = folder + stem + suffix[component & 3] + std::to_string(file_index);
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return fail(PICSONG_ERR_IO, "cannot open LUT file %s", path.c_str());
    int i = base, prev = -1, lvl, sb, bp, v[16];
    for (;;) {
        if (fscanf(f, "%d %d %d :", &lvl, &sb, &bp) != 3) break;
        bool ok = true;
        for (int c = 0; c < C; c++)
            if (fscanf(f, "%d", &v[c]) != 1) { ok = false; break; }
        if (!ok) break;
        if (bp <= prev) {
            // remaining planes of the previous group get the 7-bit mid value (IOManager.ipp:459)
            for (int z = 0; z < (nBp - prev - 1) * C; z++) {
                size_t at = (size_t)(i + prev * C + z + C);
                if (at < cap) T[at] = 64;
            }
            i += nBp * C;
        }
        if ((lvl + 1) > wl && sb > 0) break;
        prev = bp;
        for (int c = 0; c < C; c++) {
            size_t at = (size_t)(i + bp * C + c);
            if (at < cap) T[at] = v[c];
        }
    }
    fclose(f);
    return PICSONG_OK;
}

int picsong_lut_load(const char *folder_c, int component, int wl, int fill, picsong_lut_info *info,
                     int32_t *table, size_t cap)
{
    return picsong_lut_load_k(folder_c, component, wl, fill, 1, info, table, cap);
}

int picsong_lut_load_k(const char *folder_c, int component, int wl, int fill, int n_tables, picsong_lut_info *info,
                       int32_t *table, size_t cap)
{
    if (!folder_c || !info) return fail(PICSONG_ERR_ARG, "lut_load: null argument");
    if (wl < 1 || wl > 10) return fail(PICSONG_ERR_ARG, "lut_load: wl %d out of range", wl);
    std::string folder(folder_c);
    if (!folder.empty() && folder.back() != '/') folder += '/';
    FILE *f = fopen((folder + "header.txt").c_str(), "rb");
    if (!f) return fail(PICSONG_ERR_IO, "cannot open %sheader.txt", folder.c_str());
    int v[8], n = 0;
    char line[256];
    while (n < 8 && fgets(line, sizeof line, f)) {
        const char *semi = strchr(line, ';');
        if (semi) v[n++] = atoi(semi + 1);
    }
    fclose(f);
    if (n < 8) return fail(PICSONG_ERR_IO, "%sheader.txt: expected 8 KEY;value lines", folder.c_str());
    info->n_bitplanes = v[0]; info->n_subbands = v[1]; info->ctx_ref = v[2]; info->ctx_sign = v[3];
    info->ctx_sig = v[4]; info->precision = v[5]; info->n_files = v[6];
    info->n_bp_files = v[7] > 32 ? 32 : v[7];
    const int nBp = v[0], nS = v[1];
    info->n_ref = nS * nBp * info->ctx_ref * wl + nBp * info->ctx_ref;
    info->n_sig = nS * nBp * info->ctx_sig * wl + nBp * info->ctx_sig;
    info->n_sign = nS * nBp * info->ctx_sign * wl + nBp * info->ctx_sign;
    if (n_tables <= 0) n_tables = info->n_bp_files;
    if (n_tables < 1) n_tables = 1;
    info->n_tables = n_tables;
    info->cp = 2;
    if (!table) return PICSONG_OK;
    const size_t total = (size_t)info->n_ref + info->n_sig + info->n_sign;
    if (cap < total * (size_t)n_tables)
        return fail(PICSONG_ERR_ARG, "lut_load: table capacity %zu < %zu", cap, total * (size_t)n_tables);
    if (info->ctx_ref > 16 || info->ctx_sig > 16 || info->ctx_sign > 16)
        return fail(PICSONG_ERR_ARG, "lut_load: context counts above 16 are not supported");
    for (size_t i = 0; i < total * (size_t)n_tables; i++) table[i] = fill;
    for (int j = 0; j < n_tables; j++) {
        int32_t *T = table + (size_t)j * total;
        // a group-change fill may reach past its table: inside the array it lands in the next table
        // (which is parsed afterwards), at the very end it is dropped -- as in the oracle
        const size_t room = total * (size_t)(n_tables - j);
        int rc;
        if ((rc = lut_section(folder, "ref", component, j, info->ctx_ref, nBp, wl, T, 0, room))) return rc;
        if ((rc = lut_section(folder, "sig", component, j, info->ctx_sig, nBp, wl, T, info->n_ref, room))) return rc;
        if ((rc = lut_section(folder, "sign", component, j, info->ctx_sign, nBp, wl, T, info->n_ref + info->n_sig,
                              room))) return rc;
    }
    return PICSONG_OK;
}

int picsong_lut_load_cp(const char *folder_c, int component, int wl, int fill, int cp, picsong_lut_info *info,
                        int32_t *table, size_t cap)
{
    if (cp != 3) {
        const int rc = picsong_lut_load_k(folder_c, component, wl, fill, 1, info, table, cap);
        if (rc == PICSONG_OK) info->cp = 2;
        return rc;
    }
    if (!folder_c || !info) return fail(PICSONG_ERR_ARG, "lut_load: null argument");
    int rc = picsong_lut_load_k(folder_c, component, wl, fill, 1, info, nullptr, 0);      // header + section sizes
    if (rc) return rc;
    info->cp = 3;
    if (!table) return PICSONG_OK;
    const size_t b3 = (size_t)info->n_ref + info->n_sig + info->n_sign, total = b3 + info->n_sig + info->n_sign;
    if (cap < total) return fail(PICSONG_ERR_ARG, "lut_load: table capacity %zu < %zu", cap, total);
    std::string folder(folder_c);
    if (!folder.empty() && folder.back() != '/') folder += '/';
    for (size_t i = 0; i < total; i++) table[i] = fill;
    const int nBp = info->n_bitplanes;
    if ((rc = lut_section(folder, "ref", component, 0, info->ctx_ref, nBp, wl, table, 0, total))) return rc;
    if ((rc = lut_section(folder, "sig", component, 0, info->ctx_sig, nBp, wl, table, info->n_ref, total))) return rc;
    if ((rc = lut_section(folder, "sign", component, 0, info->ctx_sign, nBp, wl, table, info->n_ref + info->n_sig, total))) return rc;
    if ((rc = lut_section(folder, "cp_sig", component, 0, info->ctx_sig, nBp, wl, table, (int)b3, total))) return rc;
    if ((rc = lut_section(folder, "cp_sign", component, 0, info->ctx_sign, nBp, wl, table, (int)b3 + info->n_sig, total))) return rc;
    return PICSONG_OK;
}

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
// What a context derives from its qs (and its geometry): picsong_ctx_create and picsong_ctx_set_qs
static void ctx_derive_qs(picsong_ctx *c)
{
    const picsong_params *p = &c->p;
    c->fast_div = p->lossy != 0 && dequant_fast_ok(p->qs, p->wl);
    // 8-bit samples: 128 after the level shift; 255 covers the chroma differences of the RGB path's RCT
    c->c16 = p->bit_depth == 8 && dwt_c16_geometry_ok(c->aw, c->ah, p->wl) &&
             coef16_ok(p->lossy != 0, p->wl, p->qs, p->is_rgb ? 255 : 128);
    // (an RGB context: picsong_decode_rgb_frame's three components; the plane-by-plane calls keep the 32-bit arrays)
    c->c16_dec = p->cp != 3 && p->bit_depth == 8 &&
                 dec_c16_ok(p->lossy != 0, p->wl, p->qs, p->is_rgb ? 255 : 128, c->aw, c->ah, c->fast_div);
}

int picsong_ctx_create(const picsong_params *p, int device, picsong_ctx **out)
{
    if (!p || !out) return fail(PICSONG_ERR_ARG, "ctx_create: null argument");
    *out = nullptr;
    // Launcher.cu:132 validation + header limits
    if (p->width <= 0 || p->height <= 0) return fail(PICSONG_ERR_ARG, "xSize/ySize must be positive");
    if (p->wl < 1 || p->wl > 7) return fail(PICSONG_ERR_ARG, "wl %d outside 1..7", p->wl);
    if (p->cp != 2 && p->cp != 3) return fail(PICSONG_ERR_ARG, "cp %d: 2 or 3 coding passes", p->cp);
    if (p->cp == 3 && p->k > 0.0f) return fail(PICSONG_ERR_ARG, "-cp 3 has no complexity-scalable mode (k must be 0)");
    if (!(p->k >= 0.0f && p->k <= 65.535f)) return fail(PICSONG_ERR_ARG, "k %g outside [0, 65.535]", p->k);
    if (p->lossy && !(p->qs > 0.0f && p->qs <= 1.0f)) return fail(PICSONG_ERR_ARG, "qs %g outside (0,1]", p->qs);
    if (p->bit_depth < 8 || p->bit_depth > 16) return fail(PICSONG_ERR_ARG, "bit depth %d outside 8..16", p->bit_depth);
    if (!((p->components == 1 && !p->is_rgb) || (p->components == 3 && p->is_rgb)))
        return fail(PICSONG_ERR_ARG, "components must be 1 (grey) or 3 with is_rgb (got %d, is_rgb %d)", p->components,
                    p->is_rgb);
    // header field widths (BitStreamBuilder.cpp:54-93): height 16 bits, frames 17 bits, samples 32 bits
    if (p->height > 65535) return fail(PICSONG_ERR_ARG, "ySize %d exceeds the header's 16 bits", p->height);
    if (p->frames < 0 || p->frames >= (1 << 17)) return fail(PICSONG_ERR_ARG, "frames %d outside the header's 17 bits", p->frames);
    if ((uint64_t)p->width * (uint64_t)p->height * (uint64_t)p->components >= ((uint64_t)1 << 32))
        return fail(PICSONG_ERR_ARG, "xSize * ySize * components exceeds the header's 32 bits");
    const int aw = picsong_pad_dim(p->width), ah = picsong_pad_dim(p->height);
    // the mirror padding of IOManager::loadFrameCAdaptedSizes is only defined while the added columns / rows
    // do not outnumber the frame's own (picsong_pad_frame_host)
    if (aw - p->width > p->width || ah - p->height > p->height)
        return fail(PICSONG_ERR_ARG, "frame %dx%d is too small to be mirror-padded to %dx%d", p->width, p->height, aw, ah);
    if ((aw >> (p->wl - 1)) < 4 || (ah >> (p->wl - 1)) < 4 || ((aw >> (p->wl - 1)) & 1) || ((ah >> (p->wl - 1)) & 1))
        return fail(PICSONG_ERR_ARG, "image %dx%d too small for %d wavelet levels", aw, ah, p->wl);
    if ((size_t)aw * (size_t)ah >= ((size_t)1 << 30)) return fail(PICSONG_ERR_ARG, "frame too large");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(PICSONG_ERR_NODEVICE, "no HIP device: this library has no CPU path");
    if (device < 0 || device >= ndev) return fail(PICSONG_ERR_ARG, "device %d of %d", device, ndev);
    HIP_TRY(hipSetDevice(device));

    picsong_ctx *c = new picsong_ctx();
    memset(c, 0, sizeof *c);
    c->p = *p;
    c->device = device;
    c->aw = aw; c->ah = ah;
    c->ncb = (aw / PICSONG_CB) * (ah / PICSONG_CB);
    c->P = (size_t)aw * (size_t)ah;
    c->extra = picsong_dwt_extra(aw, ah, p->wl);
    c->dec_waves = window_waves_cap(aw, ah, p->wl, p->lossy != 0, c->ncb, kBpcEncWgWaves);
    ctx_derive_qs(c);
    c->bulk_compact[0] = c->bulk_compact[1] = c->bulk_compact[2] = -1;
    hipError_t e = hipMalloc(&c->one.offsets, sizeof(int32_t) * (size_t)c->ncb);
    if (e == hipSuccess) e = hipMalloc(&c->one.total, sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&c->d_flag, sizeof(int));
    if (e == hipSuccess) e = hipHostMalloc(&c->h_pinned, 2 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(c->d_flag, 0, sizeof(int));
    if (e == hipSuccess) e = hipMemset(c->one.total, 0, sizeof(int32_t));
    if (e != hipSuccess) {
        picsong_ctx_destroy(c);
        return fail(PICSONG_ERR_HIP, "ctx_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return PICSONG_OK;
}

static void free_workspace(Workspace &w)
{
    void *const p[] = { w.coef, w.staging, w.sizes, w.offsets, w.total, w.plane_scratch, w.coef_i };
    for (void *q : p) if (q) (void)hipFree(q);
    w = Workspace();
}

static void free_batch(picsong_ctx *c)
{
    free_workspace(c->batch);
    if (c->h_totals) (void)hipHostFree(c->h_totals);
    c->h_totals = nullptr; c->batch_cap = 0; c->b_coef_i_cap = 0;
}

void picsong_ctx_destroy(picsong_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (int k = 0; k < 3; k++)
        if (c->d_lut[k] && !c->lut_borrowed[k]) (void)hipFree(c->d_lut[k]);
    for (int k = 0; k < 3; k++)
        if (c->d_img[k]) (void)hipFree(c->d_img[k]);
    if (c->d_flag) (void)hipFree(c->d_flag);
    if (c->h_pinned) (void)hipHostFree(c->h_pinned);
    free_workspace(c->one);
    free_batch(c);
    for (int k = 0; k < 3; k++) if (c->d_train[k]) (void)hipFree(c->d_train[k]);
    if (c->train_scratch) (void)hipFree(c->train_scratch);
    if (c->rate_coef) (void)hipFree(c->rate_coef);
    if (c->q_pix) (void)hipFree(c->q_pix);
    if (c->d_sse) (void)hipFree(c->d_sse);
    if (c->h_sse) (void)hipHostFree(c->h_sse);
    if (c->lay_buf) (void)hipFree(c->lay_buf);
    if (c->prof_ev) {
        for (hipEvent_t e : *c->prof_ev) (void)hipEventDestroy(e);
        delete c->prof_ev;
    }
    delete c;
}

static LutGeo lut_geo(const picsong_lut_info &li)
{
    return lut_geo(li.n_bitplanes, li.n_subbands, li.ctx_ref, li.ctx_sign, li.ctx_sig, li.precision, li.n_ref, li.n_sig, li.n_sign);
}

// The refusals both setters share, in the order they are made.  About the caller's arguments:
static int lut_args_ok(const picsong_ctx *c, int comp, const picsong_lut_info *info, const int32_t *table, const char *who)
{
    if (!c || !info || !table) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    if (comp < 0 || comp > 2) return fail(PICSONG_ERR_ARG, "%s: component %d outside 0..2", who, comp);
    // the context formation of BPCEngine.cu:222-308 is fixed to 9 / 4 / 1 contexts
    if (info->ctx_sig != 9 || info->ctx_sign != 4 || info->ctx_ref != 1)
        return fail(PICSONG_ERR_ARG, "LUT contexts must be 9/4/1 (sig/sign/ref), got %d/%d/%d", info->ctx_sig,
                    info->ctx_sign, info->ctx_ref);
    if (info->precision < 1 || info->precision > 8) return fail(PICSONG_ERR_ARG, "LUT precision %d", info->precision);
    return PICSONG_OK;
}
// ... about one table's entries (*one) against the coders' LDS copy:
static int lut_fits_lds(const picsong_ctx *c, const picsong_lut_info &li, size_t *one)
{
    const bool cp3 = c->p.cp == 3;
    *one = (size_t)li.n_ref + (cp3 ? 2 : 1) * ((size_t)li.n_sig + li.n_sign);
    if (*one + (size_t)kLutSlack > (size_t)(cp3 ? kLutLdsMax3 : kLutLdsMax))
        return fail(PICSONG_ERR_ARG, "LUT table of %zu entries exceeds the %d the coder kernels hold in LDS", *one,
                    (cp3 ? kLutLdsMax3 : kLutLdsMax) - kLutSlack);
    return PICSONG_OK;
}
// ... and the geometry checks (lut_refusal, bpc_kernels.hpp): run before the context's table is replaced
static int lut_admit(const picsong_ctx *c, const picsong_lut_info &li, int n_tables)
{
    char msg[320];
    if (lut_refusal(lut_geo(li), c->p.wl, c->p.k > 0.0f, c->p.cp == 3, n_tables, msg, sizeof msg))
        return fail(PICSONG_ERR_ARG, "%s", msg);
    return PICSONG_OK;
}

// The k = 0 encoder's image of component comp's table (bpc_kernels.hpp, plane records).  A host table's records are
// built here, once, when the context takes it; a caller's device table may change under the context as it always
// could, so its records are rebuilt from it by one small block ahead of every encoder launch, on that launch's stream
// (plane_img_refresh).  Contexts that code with -k > 0 or -cp 3 keep no image.
static bool ctx_uses_plane_img(const picsong_ctx *c) { return !(c->p.k > 0.0f) && c->p.cp != 3; }
static int plane_img_alloc(picsong_ctx *c, int comp)
{
    if (!c->d_img[comp]) HIP_TRY(hipMalloc(&c->d_img[comp], kPlaneImgMaxRecs * sizeof(PlaneRec)));
    return PICSONG_OK;
}
static int plane_img_from_host(picsong_ctx *c, int comp, const picsong_lut_info &li, const int32_t *host_table)
{
    if (!ctx_uses_plane_img(c)) return PICSONG_OK;
    if (int rc = plane_img_alloc(c, comp)) return rc;
    const LutGeo g = lut_geo(li);
    std::vector<PlaneRec> img((size_t)plane_img_recs(c->p.wl));
    for (size_t i = 0; i < img.size(); i++) img[i] = plane_record(host_table, g, (int)i / kMaxPlanes, (int)i % kMaxPlanes);
    HIP_TRY(hipMemcpy(c->d_img[comp], img.data(), img.size() * sizeof(PlaneRec), hipMemcpyHostToDevice));
    return PICSONG_OK;
}
// ahead of a k = 0 encoder launch on stream s
static int plane_img_refresh(picsong_ctx *c, int comp, hipStream_t s)
{
    if (!ctx_uses_plane_img(c) || !c->lut_borrowed[comp]) return PICSONG_OK;
    return HipGo{ s }(plane_img_kernel, dim3(1), 256u, c->d_lut[comp], lut_geo(c->li[comp]), c->p.wl, c->d_img[comp]);
}

int picsong_ctx_set_lut_component(picsong_ctx *c, int comp, const picsong_lut_info *info, const int32_t *host_table)
{
    if (int rc = lut_args_ok(c, comp, info, host_table, "set_lut")) return rc;
    const bool cp3 = c->p.cp == 3;
    if (cp3 != (info->cp == 3))
        return fail(PICSONG_ERR_ARG, "the context codes %d passes, the table is laid out for %d (picsong_lut_load_cp)",
                    c->p.cp, info->cp == 3 ? 3 : 2);
    const int n_tables = info->n_tables > 0 ? info->n_tables : 1;
    size_t one;
    if (int rc = lut_fits_lds(c, *info, &one)) return rc;
    const size_t total = one * (size_t)n_tables;
    for (size_t i = 0; i < total; i++)
        if (host_table[i] < 0 || host_table[i] > 255)
            return fail(PICSONG_ERR_ARG, "LUT entry %zu = %d outside 0..255", i, host_table[i]);
    if (int rc = lut_admit(c, *info, n_tables)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = plane_img_from_host(c, comp, *info, host_table)) return rc;
    if (c->d_lut[comp] && !c->lut_borrowed[comp]) (void)hipFree(c->d_lut[comp]);
    c->d_lut[comp] = nullptr;
    c->lut_borrowed[comp] = false;
    HIP_TRY(hipMalloc(&c->d_lut[comp], total * sizeof(int32_t)));
    HIP_TRY(hipMemcpy(c->d_lut[comp], host_table, total * sizeof(int32_t), hipMemcpyHostToDevice));
    c->li[comp] = *info;
    c->li[comp].n_tables = n_tables;
    c->has_lut[comp] = true;
    c->bulk_compact[comp] = -1;
    return PICSONG_OK;
}

int picsong_ctx_set_lut_device(picsong_ctx *c, int comp, const picsong_lut_info *info, const int32_t *d_table)
{
    if (int rc = lut_args_ok(c, comp, info, d_table, "set_lut_device")) return rc;
    picsong_lut_info li = *info;
    // section sizes follow from the geometry (IO/IOManager.ipp:431-433) when the caller left them 0
    const int wl = c->p.wl;
    if (li.n_ref <= 0) li.n_ref = li.n_subbands * li.n_bitplanes * li.ctx_ref * wl + li.n_bitplanes * li.ctx_ref;
    if (li.n_sig <= 0) li.n_sig = li.n_subbands * li.n_bitplanes * li.ctx_sig * wl + li.n_bitplanes * li.ctx_sig;
    if (li.n_sign <= 0) li.n_sign = li.n_subbands * li.n_bitplanes * li.ctx_sign * wl + li.n_bitplanes * li.ctx_sign;
    // the borrowed table is laid out for the context's coding passes: [ref | sig | sign] for -cp 2, the five sections
    // [ref | sig | sign | cp_sig | cp_sign] for -cp 3 (what bpc3_kernel copies to LDS); `info->cp` as the façade's
    // geometry() leaves it (0) means "the context's"; a table declared for the other mode is refused
    const bool cp3 = c->p.cp == 3;
    if (info->cp != 0 && cp3 != (info->cp == 3))
        return fail(PICSONG_ERR_ARG, "the context codes %d passes, the device table is laid out for %d", c->p.cp,
                    info->cp == 3 ? 3 : 2);
    li.cp = c->p.cp;
    size_t one;
    if (int rc = lut_fits_lds(c, li, &one)) return rc;
    if (li.n_tables <= 0) li.n_tables = 1;
    if (int rc = lut_admit(c, li, li.n_tables)) return rc;
    if (ctx_uses_plane_img(c)) {
        HIP_TRY(hipSetDevice(c->device));
        if (int rc = plane_img_alloc(c, comp)) return rc;
    }
    if (c->d_lut[comp] && !c->lut_borrowed[comp]) (void)hipFree(c->d_lut[comp]);
    c->d_lut[comp] = const_cast<int32_t *>(d_table);
    c->lut_borrowed[comp] = true;
    c->li[comp] = li;
    c->has_lut[comp] = true;
    c->bulk_compact[comp] = -1;
    return PICSONG_OK;
}

int picsong_ctx_set_lut(picsong_ctx *c, const picsong_lut_info *info, const int32_t *host_table)
{
    return picsong_ctx_set_lut_component(c, 0, info, host_table);
}

int picsong_ctx_set_pipelined(picsong_ctx *c, int on)
{
    if (!c) return fail(PICSONG_ERR_ARG, "set_pipelined: null context");
    c->pipelined = on != 0;
    return PICSONG_OK;
}

int picsong_ctx_set_decode_drop(picsong_ctx *c, int drop)
{
    if (!c) return fail(PICSONG_ERR_ARG, "set_decode_drop: null context");
    if (!drop_ok(drop)) return fail(PICSONG_ERR_ARG, "set_decode_drop: drop %d outside 0..%d", drop, kDropMax);
    if (c->p.k > 0.0f) return fail(PICSONG_ERR_ARG, "set_decode_drop: a -k > 0 context codes the planes below cbp in its bulk scan");
    if (c->p.cp == 3) return fail(PICSONG_ERR_ARG, "set_decode_drop: a -cp 3 context codes a plane in three passes");
    c->drop = drop;
    return PICSONG_OK;
}

int picsong_ctx_get_decode_drop(const picsong_ctx *c, int *drop)
{
    if (!c || !drop) return fail(PICSONG_ERR_ARG, "get_decode_drop: null argument");
    *drop = c->drop;
    return PICSONG_OK;
}

int picsong_drop_planes(int aw, int ah, int wl, int drop, int cb, int *planes)
{
    if (!planes) return fail(PICSONG_ERR_ARG, "drop_planes: null argument");
    if (aw < PICSONG_CB || ah < PICSONG_CB || aw % PICSONG_CB || ah % PICSONG_CB)
        return fail(PICSONG_ERR_ARG, "drop_planes: %d x %d is no padded size (positive multiples of %d)", aw, ah, PICSONG_CB);
    if (wl < 1 || wl > 7) return fail(PICSONG_ERR_ARG, "drop_planes: wl %d outside 1..7", wl);
    if (!drop_ok(drop)) return fail(PICSONG_ERR_ARG, "drop_planes: drop %d outside 0..%d", drop, kDropMax);
    if (cb < 0 || cb >= (aw / PICSONG_CB) * (ah / PICSONG_CB))
        return fail(PICSONG_ERR_ARG, "drop_planes: codeblock %d outside 0..%d", cb, (aw / PICSONG_CB) * (ah / PICSONG_CB) - 1);
    *planes = drop_planes_of(aw, ah, wl, drop, cb);
    return PICSONG_OK;
}

int picsong_ctx_set_qs(picsong_ctx *c, float qs)
{
    if (!c) return fail(PICSONG_ERR_ARG, "set_qs: null context");
    if (!(qs > 0.0f)) return fail(PICSONG_ERR_ARG, "set_qs: qs %g must be positive", qs);
    // (picsong_ctx_create keeps the coding launcher's (0, 1]; here every gain the header's 14 bits store is taken, up to
    // q(16383): the rate search's grid, and what a decoder may meet in a stream)
    if (!(qs <= rate_q(kRateJMax))) return fail(PICSONG_ERR_ARG, "set_qs: qs %g is beyond the header's range (0, %g]", qs, rate_q(kRateJMax));
    c->p.qs = qs;
    ctx_derive_qs(c);
    return PICSONG_OK;
}

int picsong_rate_qs(int j, float *qs)
{
    if (!qs) return fail(PICSONG_ERR_ARG, "rate_qs: null argument");
    if (!rate_header_exact(j))
        return fail(PICSONG_ERR_ARG, "rate_qs: j = %d is outside 1..%d or not stored exactly by the header", j, kRateJMax);
    *qs = rate_q(j);
    return PICSONG_OK;
}

int picsong_ctx_padded_dims(const picsong_ctx *c, int *aw, int *ah, int *ncb)
{
    if (!c) return fail(PICSONG_ERR_ARG, "null ctx");
    if (aw) *aw = c->aw;
    if (ah) *ah = c->ah;
    if (ncb) *ncb = c->ncb;
    return PICSONG_OK;
}

// ---------------------------------------------------------------------------------------------
// level shift
// ---------------------------------------------------------------------------------------------
int picsong_level_shift_fwd(picsong_ctx *c, const uint8_t *d_in, void *d_out, void *stream)
{
    REFUSE_DEEP(c, "level_shift_fwd");
    if (!c || !d_in || !d_out) return fail(PICSONG_ERR_ARG, "level_shift_fwd: null argument");
    return level_shift_fwd(HipGo{ (hipStream_t)stream }, c->p.lossy != 0, d_in, d_out, c->P / 4, level_off(c));
}

int picsong_level_shift_inv(picsong_ctx *c, void *d_data, void *stream)
{
    if (!c || !d_data) return fail(PICSONG_ERR_ARG, "level_shift_inv: null argument");
    if (is_deep(c)) return level_shift_inv16(HipGo{ (hipStream_t)stream }, c->p.lossy != 0, d_data, c->P, level_off(c), px_max(c));
    return level_shift_inv(HipGo{ (hipStream_t)stream }, c->p.lossy != 0, d_data, c->P, level_off(c));
}

// ---------------------------------------------------------------------------------------------
// DWT
// ---------------------------------------------------------------------------------------------
// want_c16: the context's choice of the 16-bit coefficient form (picsong_ctx::c16); *got_c16: what THIS call's plan
// delivers -- the form exists in the vector kernels only, and whether those apply also depends on the caller's pointers
// (16-byte alignment) and on PICSONG_DWT_NOVEC at call time, so a call may fall back to the 32-bit arrays and the
// coder must be told (plan_dwt_forward clears c16 on every level then)
static int dwt_forward_impl(picsong_ctx *c, const void *d_in, bool u8in, void *d_out, hipStream_t s, bool want_c16 = false,
                            bool *got_c16 = nullptr)
{
    const std::vector<FwdLaunch> plan = plan_dwt_forward(d_in, u8in, d_out, c->aw, c->ah, c->p.wl, c->p.qs, want_c16);
    if (got_c16) *got_c16 = plan_is_c16(plan);
    else if (want_c16 && !plan_is_c16(plan)) return fail(PICSONG_ERR_ARG, "the 16-bit coefficient form needs the vector kernels on every level");
    return launch_fwd_plan(HipGo{ s }, c->p.lossy != 0, plan);
}

int picsong_dwt_forward(picsong_ctx *c, const void *d_in, void *d_out, void *stream)
{
    if (!c || !d_in || !d_out) return fail(PICSONG_ERR_ARG, "dwt_forward: null argument");
    return dwt_forward_impl(c, d_in, false, d_out, (hipStream_t)stream);
}

int picsong_dwt_forward_u8(picsong_ctx *c, const uint8_t *d_in, void *d_out, void *stream)
{
    REFUSE_DEEP(c, "dwt_forward_u8");
    if (!c || !d_in || !d_out) return fail(PICSONG_ERR_ARG, "dwt_forward_u8: null argument");
    return dwt_forward_impl(c, d_in, true, d_out, (hipStream_t)stream);
}

int picsong_dwt_forward_band(picsong_ctx *c, const uint8_t *d_frame, int row0, int rows, void *d_out, void *stream)
{
    REFUSE_DEEP(c, "dwt_forward_band");
    if (!c || !d_frame || !d_out) return fail(PICSONG_ERR_ARG, "dwt_forward_band: null argument");
    if (row0 < 0 || rows <= 0 || (row0 & 1) || (rows & 1) || row0 + rows > c->ah)
        return fail(PICSONG_ERR_ARG, "dwt_forward_band: rows [%d, %d) must be even and inside [0, %d)", row0, row0 + rows, c->ah);
    std::vector<FwdLaunch> plan = plan_dwt_forward(d_frame, true, d_out, c->aw, c->ah, c->p.wl, c->p.qs);
    plan_restrict_band(plan[0], row0, rows);
    plan.resize(1);
    return launch_fwd_levels(HipGo{ (hipStream_t)stream }, c->p.lossy != 0, plan, 0);
}

int picsong_dwt_forward_tail(picsong_ctx *c, void *d_out, void *stream)
{
    if (!c || !d_out) return fail(PICSONG_ERR_ARG, "dwt_forward_tail: null argument");
    // (the level-0 source is irrelevant here: only the launches of levels >= 1 are used)
    const std::vector<FwdLaunch> plan = plan_dwt_forward(d_out, false, d_out, c->aw, c->ah, c->p.wl, c->p.qs);
    return launch_fwd_levels(HipGo{ (hipStream_t)stream }, c->p.lossy != 0, plan, 1);
}

int picsong_dwt_inverse(picsong_ctx *c, const int32_t *d_in, void *d_out, void *stream)
{
    if (!c || !d_in || !d_out) return fail(PICSONG_ERR_ARG, "dwt_inverse: null argument");
    // (32-bit coefficients, no pixels: a launch per level, plan_dwt_inv2 never applies)
    return run_inverse(HipGo{ (hipStream_t)stream }, c->p.lossy != 0, lean97_levels(),
                       plan_dwt_inverse(d_in, d_out, c->aw, c->ah, c->p.wl, c->p.qs, c->fast_div));
}

// ---------------------------------------------------------------------------------------------
// BPC
// ---------------------------------------------------------------------------------------------
static int bpc_args(picsong_ctx *c, BpcArgs &a, int comp = 0)
{
    if (comp < 0 || comp > 2) return fail(PICSONG_ERR_ARG, "component %d outside 0..2", comp);
    if (!c->has_lut[comp]) return fail(PICSONG_ERR_ARG, "no LUT loaded for component %d: call picsong_ctx_set_lut first", comp);
    const picsong_lut_info &li = c->li[comp];
    a = bpc_frame_args(c->aw, c->ah, c->p.wl, c->d_lut[comp], lut_geo(li), c->d_flag);
    a.plane_img = ctx_uses_plane_img(c) ? c->d_img[comp] : nullptr;
    a.k = c->p.k; a.n_tables = li.n_tables > 0 ? li.n_tables : 1;
    a.drop = c->drop;                                       // (the decoders' alone: launch_decoder)
    return PICSONG_OK;
}

// -k > 0: may a launch over the tables of components comp .. comp + ncomp - 1 take the kernels' COMPACT table copies
// (bulk_compact, kernel_select.hpp)?  PICSONG_BULK_FULLTAB=1 keeps the whole-table instantiations (the tests cross-check both)
static bool bulk_compact(picsong_ctx *c, int comp, int ncomp = 1)
{
    if (const char *e = getenv("PICSONG_BULK_FULLTAB")) if (atoi(e) != 0) return false;
    for (int k = comp; k < comp + ncomp; k++) {
        if (c->bulk_compact[k] < 0) c->bulk_compact[k] = picsong::bulk_compact(c->aw, c->ah, c->p.wl, lut_geo(c->li[k])) ? 1 : 0;
        if (c->bulk_compact[k] != 1) return false;
    }
    return true;
}

// the waves of a frame's coder launch the bit-plane scratch holds, whole workgroups: every codeblock pair, or the most a
// window call lists (window_waves_cap: a codeblock that straddles subbands may be listed twice)
static int dec_scratch_waves(const picsong_ctx *c) { return c->dec_waves; }
// the coders' bit-plane scratch: kEncScratchDwordsPerWave per wave of a frame's launch (whole workgroups), allocated
// at the first use
static int ensure_plane_scratch(picsong_ctx *c)
{
    static_assert(kBpcEncWgWaves == kBpcDecWgWaves, "one scratch serves the launches of both directions");
    static_assert(kBpcEncWgWaves % kBpc3WgWaves == 0, "-cp 3 launches fit the same allocation");
    if (c->one.plane_scratch) return PICSONG_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMalloc(&c->one.plane_scratch, (size_t)dec_scratch_waves(c) * kEncScratchDwordsPerWave * sizeof(uint32_t)));
    return PICSONG_OK;
}

// The encoder launch of every path: `waves` waves (a codeblock pair each) over the tables of components comp ..
// comp + ncomp - 1, the caller's `a` complete but for the kernel's choice.  Ahead of a k = 0 launch the plane records of
// a caller's device tables are rebuilt (plane_img_refresh).
static int launch_encoder(picsong_ctx *c, const BpcArgs &a, unsigned waves, int comp, int ncomp, hipStream_t s)
{
    const bool bulk = a.k > 0.0f;
    if (!bulk)
        for (int k = comp; k < comp + ncomp; k++) if (int rc = plane_img_refresh(c, k, s)) return rc;
    return picsong::launch_encoder(HipGo{ s }, a, c->p.cp == 3, bulk && bulk_compact(c, comp, ncomp) && c->pipelined, waves);
}

// d_stage16: the encoders' 16-bit staging, uint16[nCB * 4096] (BpcArgs::staging16) -- the context's own staging
// buffers hold it on the frame paths; picsong_bpc_encode widens it into the caller's int32 array
static int bpc_encode_impl(picsong_ctx *c, const void *d_coeffs, uint16_t *d_stage16, int32_t *d_sizes,
                           hipStream_t s, int cb_begin = 0, int cb_count = -1, int comp = 0, bool c16 = false)
{
    BpcArgs a;
    int rc = bpc_args(c, a, comp);
    if (rc) return rc;
    a.c16 = c16 ? 1 : 0;
    if (cb_count < 0) cb_count = c->ncb - cb_begin;
    a.cb_base = cb_begin;
    a.nCB = cb_begin + cb_count;
    a.coeffs_in = d_coeffs; a.is_float = c->p.lossy ? 1 : 0;
    a.staging16 = d_stage16; a.sizes = d_sizes;
    if (int rc2 = ensure_plane_scratch(c)) return rc2;
    a.plane_scratch = c->one.plane_scratch;
    return launch_encoder(c, a, (unsigned)((cb_count + 1) / 2), comp, 1, s);
}

// The stage-level call keeps the reference's contract -- an int32 array of 4096 words a codeblock, 0xFFFFFFFF wherever
// nothing was written (BPCEngine::deviceMemoryAllocator BPCEngine.cu:2429-2441) -- on top of the encoders' 16-bit
// staging: the coder writes the context's own buffer, widen_staging_kernel copies words 0 .. len - 1 of every codeblock.
static int bpc_encode_widened(picsong_ctx *c, const void *d_coeffs, int32_t *d_staging, int32_t *d_sizes, hipStream_t s, int comp)
{
    HIP_TRY(hipSetDevice(c->device));
    if (!c->one.staging) HIP_TRY(hipMalloc(&c->one.staging, c->P * sizeof(int32_t)));
    if (d_staging == c->one.staging) return fail(PICSONG_ERR_ARG, "bpc_encode: the context's own staging passed as the output");
    uint16_t *const st16 = reinterpret_cast<uint16_t *>(c->one.staging);
    HIP_TRY(hipMemsetAsync(d_staging, 0xFF, c->P * sizeof(int32_t), s));
    int rc = bpc_encode_impl(c, d_coeffs, st16, d_sizes, s, 0, -1, comp);
    if (rc) return rc;
    return widen_staging(HipGo{ s }, st16, d_sizes, 0, c->ncb, d_staging);
}

int picsong_bpc_encode(picsong_ctx *c, const void *d_coeffs, int32_t *d_staging, int32_t *d_sizes, void *stream)
{
    if (!c || !d_coeffs || !d_staging || !d_sizes) return fail(PICSONG_ERR_ARG, "bpc_encode: null argument");
    return bpc_encode_widened(c, d_coeffs, d_staging, d_sizes, (hipStream_t)stream, 0);
}

// PICSONG_DEC_STAGING=1: the frame paths unpack into the 32-bit staging first, as picsong_bitstream_unpack +
// picsong_bpc_decode do (A/B of the decoder that reads the stream itself)
static bool dec_from_stream(const picsong_ctx *c)
{
    static const bool staged = [] { const char *e = getenv("PICSONG_DEC_STAGING"); return e && atoi(e) != 0; }();
    return !staged && c->p.cp != 3;
}

// Stream intake (launch_seq.hpp) of n streams `stride` shorts apart into w
static int stream_intake(picsong_ctx *c, const uint16_t *d_streams, unsigned n, size_t stride, bool direct, const Workspace &w,
                         hipStream_t s)
{
    return picsong::stream_intake(HipGo{ s }, d_streams, n, stride, direct, c->ncb, c->P, w, c->d_flag);
}

// a decoder launch refused (kLaunchRefused, launch_seq.hpp) as the ABI's error
static int refused_rc(int rc)
{
    return rc == kLaunchRefused ? fail(PICSONG_ERR_ARG, "the 16-bit coefficient form decodes from the stream itself") : rc;
}

// One plane's decoder (the stage calls, picsong_decode_plane) over the context's own scratch: every codeblock, 32-bit
// coefficients; d_staging / d_sizes / d_coeffs may be the caller's arrays; d_stream16: from the packed stream itself
static int bpc_decode_impl(picsong_ctx *c, const int32_t *d_staging, const int32_t *d_sizes, int32_t *d_coeffs,
                           hipStream_t s, int comp = 0, const uint16_t *d_stream16 = nullptr)
{
    BpcArgs a;
    int rc = bpc_args(c, a, comp);
    if (rc) return rc;
    if (int rc2 = ensure_plane_scratch(c)) return rc2;      // the decoder parks its finished planes there too
    Workspace w = c->one;
    w.staging = const_cast<int32_t *>(d_staging); w.sizes = const_cast<int32_t *>(d_sizes); w.coef_i = d_coeffs;
    return refused_rc(launch_decoder(HipGo{ s }, a, c->p.cp == 3, (unsigned)(c->ncb + 1) / 2, a.k > 0.0f && bulk_compact(c, comp), w,
                                     d_stream16, 0, (uint32_t)picsong_max_stream_shorts(c->aw, c->ah), false));
}

int picsong_bpc_decode(picsong_ctx *c, const int32_t *d_staging, const int32_t *d_sizes, int32_t *d_coeffs,
                       void *stream)
{
    if (!c || !d_coeffs || !d_staging || !d_sizes) return fail(PICSONG_ERR_ARG, "bpc_decode: null argument");
    return bpc_decode_impl(c, d_staging, d_sizes, d_coeffs, (hipStream_t)stream);
}

int picsong_bpc_encode_component(picsong_ctx *c, int comp, const void *d_coeffs, int32_t *d_staging, int32_t *d_sizes,
                                 void *stream)
{
    if (!c || !d_coeffs || !d_staging || !d_sizes) return fail(PICSONG_ERR_ARG, "bpc_encode: null argument");
    return bpc_encode_widened(c, d_coeffs, d_staging, d_sizes, (hipStream_t)stream, comp);
}

int picsong_bpc_decode_component(picsong_ctx *c, int comp, const int32_t *d_staging, const int32_t *d_sizes,
                                 int32_t *d_coeffs, void *stream)
{
    if (!c || !d_coeffs || !d_staging || !d_sizes) return fail(PICSONG_ERR_ARG, "bpc_decode: null argument");
    return bpc_decode_impl(c, d_staging, d_sizes, d_coeffs, (hipStream_t)stream, comp);
}

int picsong_selftest_lds_order(int device, int *mismatches)
{
    if (!mismatches) return fail(PICSONG_ERR_ARG, "selftest: null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(PICSONG_ERR_NODEVICE, "no HIP device: this library has no CPU path");
    if (device < 0 || device >= ndev) return fail(PICSONG_ERR_ARG, "device %d of %d", device, ndev);
    HIP_TRY(hipSetDevice(device));
    uint32_t *d = nullptr, h = 0;
    HIP_TRY(hipMalloc(&d, sizeof(uint32_t)));
    HIP_TRY(hipMemset(d, 0, sizeof(uint32_t)));
    const int rc = HipGo{ nullptr }(lds_order_selftest_kernel, dim3(2048), 256u, 2000, 0x5EED1234u, d);
    const hipError_t e = rc ? hipSuccess : hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (rc) return rc;
    if (e != hipSuccess) return fail(PICSONG_ERR_HIP, "selftest: %s", hipGetErrorString(e));
    *mismatches = (int)h;
    return PICSONG_OK;
}

int picsong_range_flag(picsong_ctx *c, void *stream, int *h_flag)
{
    if (!c || !h_flag) return fail(PICSONG_ERR_ARG, "range_flag: null argument");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(&c->h_pinned[1], c->d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(c->d_flag, 0, sizeof(int), s));      // read and clear: the next query covers later calls only
    HIP_TRY(hipStreamSynchronize(s));
    *h_flag = c->h_pinned[1];
    return PICSONG_OK;
}

// ---------------------------------------------------------------------------------------------
// BitStreamBuilder
// ---------------------------------------------------------------------------------------------
int picsong_last_total(picsong_ctx *c, void *stream, int *h_total)
{
    if (!c || !h_total) return fail(PICSONG_ERR_ARG, "last_total: null argument");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(&c->h_pinned[0], c->one.total, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *h_total = c->h_pinned[0];
    return PICSONG_OK;
}

extern "C++" {
// codeblocks [cb_begin, cb_begin + n) of one frame out of the context's own offsets and total
template <typename W>
static int pack_range(picsong_ctx *c, const W *d_staging, const int32_t *d_sizes, int n,
                      const uint16_t *h_header, uint16_t *d_stream, hipStream_t s)
{
    c->last_batch = 0;                                      // the most recent total is one.total (picsong_copy_last_totals)
    Workspace w = c->one;
    w.sizes = const_cast<int32_t *>(d_sizes);
    return pack_frames(HipGo{ s }, d_staging, w, n, 1u, h_header, 1, d_stream, c->P, 0);
}
}  // extern "C++"

int picsong_bitstream_pack(picsong_ctx *c, const int32_t *d_staging, const int32_t *d_sizes,
                           const uint16_t *h_header, uint16_t *d_stream, int *h_total, void *stream)
{
    if (!c || !d_staging || !d_sizes || !d_stream) return fail(PICSONG_ERR_ARG, "bitstream_pack: null argument");
    int rc = pack_range(c, d_staging, d_sizes, c->ncb, h_header, d_stream, (hipStream_t)stream);
    if (rc) return rc;
    if (h_total) return picsong_last_total(c, stream, h_total);
    return PICSONG_OK;
}

int picsong_bitstream_unpack(picsong_ctx *c, const uint16_t *d_stream, int32_t *d_staging, int32_t *d_sizes,
                             void *stream)
{
    if (!c || !d_staging || !d_sizes || !d_stream) return fail(PICSONG_ERR_ARG, "bitstream_unpack: null argument");
    // BSEngine::deviceMemoryAllocator BitStreamBuilder.cu:281-284.  Slots beyond a codeblock's length
    // are never read by the decoder, so the frame paths skip this 4*AW*AH-byte fill.
    HIP_TRY(hipMemsetAsync(d_staging, 0xFF, c->P * sizeof(int32_t), (hipStream_t)stream));
    Workspace w = c->one;
    w.staging = d_staging; w.sizes = d_sizes;
    return stream_intake(c, d_stream, 1u, 0, false, w, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// whole frame
// ---------------------------------------------------------------------------------------------
static int ensure_workspace(picsong_ctx *c, bool decode)
{
    HIP_TRY(hipSetDevice(c->device));
    Workspace &w = c->one;
    if (!w.coef) HIP_TRY(hipMalloc(&w.coef, (c->P + c->extra) * 4));
    if (!w.staging) HIP_TRY(hipMalloc(&w.staging, c->P * sizeof(int32_t)));
    if (!w.sizes) HIP_TRY(hipMalloc(&w.sizes, (size_t)c->ncb * sizeof(int32_t)));
    if (decode && !w.coef_i) HIP_TRY(hipMalloc(&w.coef_i, c->P * sizeof(int32_t)));
    return PICSONG_OK;
}

int picsong_profile_begin(picsong_ctx *c, int capacity)
{
    if (!c || capacity < 0) return fail(PICSONG_ERR_ARG, "profile_begin: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->prof_ev) c->prof_ev = new std::vector<hipEvent_t>();
    while ((int)c->prof_ev->size() < 4 * capacity) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        c->prof_ev->push_back(e);
    }
    c->prof_cap = capacity;
    c->prof_n = 0;
    return PICSONG_OK;
}

int picsong_profile_read(picsong_ctx *c, int *n_frames, float *ms, int cap)
{
    if (!c || !n_frames || !ms) return fail(PICSONG_ERR_ARG, "profile_read: null argument");
    const int n = c->prof_n < cap ? c->prof_n : cap;
    for (int f = 0; f < n; f++) {
        hipEvent_t *e = c->prof_ev->data() + 4 * f;
        HIP_TRY(hipEventSynchronize(e[3]));
        for (int k = 0; k < 3; k++) HIP_TRY(hipEventElapsedTime(&ms[3 * f + k], e[k], e[k + 1]));
    }
    *n_frames = n;
    return PICSONG_OK;
}

int picsong_encode_frame(picsong_ctx *c, const uint8_t *d_frame, int iter, uint16_t *d_stream, void *stream)
{
    REFUSE_DEEP(c, "encode_frame");
    if (!c || !d_frame || !d_stream) return fail(PICSONG_ERR_ARG, "encode_frame: null argument");
    int rc = ensure_workspace(c, false);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t *ev = nullptr;
    if (c->prof_cap > 0 && c->prof_n < c->prof_cap) ev = c->prof_ev->data() + 4 * (c->prof_n++);
    if (ev) HIP_TRY(hipEventRecord(ev[0], s));
    // (coefficients between the transform and the coder as int16 where their magnitudes are bounded: c->c16)
    // (Round 3 tried, for a lone frame, the coder's launch for the codeblock rows below AH/4 -- final once the fused head has
    // run -- at once on the caller's stream, and the transform's small levels + the coder's launch for the top rows on a
    // second stream beside it: byte-identical, and 70 us SLOWER at 8K (0.308 -> 0.379 ms): the top-left codeblocks are the
    // ones with the most planes, the launch's critical waves, and the split starts exactly those 20-40 us late.)
    // (an unaligned frame pointer, or PICSONG_DWT_NOVEC set after the context was created, takes the per-column kernels
    // and with them the 32-bit arrays: `c16` is what this call's plan delivers, as in picsong_encode_frames)
    bool c16 = false;
    if ((rc = dwt_forward_impl(c, d_frame, true, c->one.coef, s, c->c16, &c16))) return rc;
    if (ev) HIP_TRY(hipEventRecord(ev[1], s));
    uint16_t *const st16 = reinterpret_cast<uint16_t *>(c->one.staging);      // (the context's staging holds the 16-bit form)
    if ((rc = bpc_encode_impl(c, c->one.coef, st16, c->one.sizes, s, 0, -1, 0, c16))) return rc;
    if (ev) HIP_TRY(hipEventRecord(ev[2], s));
    uint16_t hdr[PICSONG_HDR_SHORTS];
    if (iter == 0) picsong_header_pack(&c->p, hdr);
    rc = pack_range(c, st16, c->one.sizes, c->ncb, iter == 0 ? hdr : nullptr, d_stream, s);
    if (ev) HIP_TRY(hipEventRecord(ev[3], s));
    return rc;
}

// The decode calls at 1/2^reduce resolution: may the decoder hand the synthesis 16-bit coefficients?  c->c16_dec
// (reduce = 0), or dec_c16_ok over the levels such a call runs.
static bool dec_c16_reduced(const picsong_ctx *c, int reduce)
{
    if (reduce == 0) return c->c16_dec;
    return c->p.cp != 3 && c->p.bit_depth == 8 &&
           dec_c16_ok(c->p.lossy != 0, c->p.wl, c->p.qs, c->p.is_rgb ? 255 : 128, c->aw, c->ah, c->fast_div, reduce);
}
// the refusals the reduced calls share (nothing is launched)
static int reduced_args_ok(const picsong_ctx *c, int reduce, const char *who)
{
    if (c->p.cp == 3) return fail(PICSONG_ERR_ARG, "%s: -cp 3 contexts have no reduced-resolution decode", who);
    if (!reduce_ok(c->p.wl, reduce))
        return fail(PICSONG_ERR_ARG, "%s: reduce %d outside 0..%d (wl - 1)", who, reduce, c->p.wl - 1);
    return PICSONG_OK;
}

int picsong_reduced_dims(const picsong_ctx *c, int reduce, int *rw, int *rh, int *paw, int *pah, int *n_codeblocks)
{
    if (!c || !rw || !rh || !paw || !pah || !n_codeblocks) return fail(PICSONG_ERR_ARG, "reduced_dims: null argument");
    if (!reduce_ok(c->p.wl, reduce))
        return fail(PICSONG_ERR_ARG, "reduced_dims: reduce %d outside 0..%d (wl - 1)", reduce, c->p.wl - 1);
    int d[5];
    reduced_dims(c->p.width, c->p.height, c->aw, c->ah, reduce, d);
    *rw = d[0]; *rh = d[1]; *paw = d[2]; *pah = d[3]; *n_codeblocks = d[4];
    return PICSONG_OK;
}

// the refusals the window calls share (nothing is launched); sets *plan
static int window_args_ok(const picsong_ctx *c, int reduce, int x, int y, int w, int h, const char *who, WindowPlan *plan)
{
    if (int rc = reduced_args_ok(c, reduce, who)) return rc;
    if (w < 1 || h < 1) return fail(PICSONG_ERR_ARG, "%s: window %d x %d is empty", who, w, h);
    const int paw = c->aw >> reduce, pah = c->ah >> reduce;
    if (!window_ok(paw, pah, x, y, w, h))
        return fail(PICSONG_ERR_ARG, "%s: window [%d, %lld) x [%d, %lld) not inside the %d x %d padded image at reduce %d", who,
                    x, (long long)x + w, y, (long long)y + h, paw, pah, reduce);
    *plan = window_plan(c->aw, c->ah, c->p.wl, c->p.lossy != 0, reduce, x, y, w, h);
    if (window_waves(*plan) > dec_scratch_waves(c))             // (cannot happen: window_waves_cap bounds every window)
        return fail(PICSONG_ERR_ARG, "%s: the window lists more codeblocks than the decoder's scratch holds", who);
    return PICSONG_OK;
}

int picsong_window_codeblocks(const picsong_ctx *c, int reduce, int x, int y, int w, int h, int *n_codeblocks)
{
    if (!c || !n_codeblocks) return fail(PICSONG_ERR_ARG, "window_codeblocks: null argument");
    WindowPlan plan;
    if (int rc = window_args_ok(c, reduce, x, y, w, h, "window_codeblocks", &plan)) return rc;
    *n_codeblocks = plan.n_cb;
    return PICSONG_OK;
}

int picsong_encode_stripe_coded(picsong_ctx *c, const void *d_coeffs, int cb_begin, int cb_count, uint16_t *d_stream,
                                void *stream)
{
    if (!c || !d_coeffs || !d_stream) return fail(PICSONG_ERR_ARG, "encode_stripe_coded: null argument");
    if (cb_begin < 0 || cb_count <= 0 || cb_begin + cb_count > c->ncb)
        return fail(PICSONG_ERR_ARG, "encode_stripe_coded: codeblocks [%d, %d) outside [0, %d)", cb_begin,
                    cb_begin + cb_count, c->ncb);
    int rc = ensure_workspace(c, false);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    uint16_t *const st16 = reinterpret_cast<uint16_t *>(c->one.staging);
    if ((rc = bpc_encode_impl(c, d_coeffs, st16, c->one.sizes, s, cb_begin, cb_count))) return rc;
    return pack_range(c, st16 + (size_t)cb_begin * PICSONG_CB_WORDS, c->one.sizes + cb_begin, cb_count, nullptr,
                      d_stream, s);
}

int picsong_encode_frame_stripe(picsong_ctx *c, const uint8_t *d_frame, int cb_begin, int cb_count,
                                uint16_t *d_stream, void *stream)
{
    REFUSE_DEEP(c, "encode_frame_stripe");
    if (!c || !d_frame || !d_stream) return fail(PICSONG_ERR_ARG, "encode_frame_stripe: null argument");
    if (cb_begin < 0 || cb_count <= 0 || cb_begin + cb_count > c->ncb)
        return fail(PICSONG_ERR_ARG, "encode_frame_stripe: codeblocks [%d, %d) outside [0, %d)", cb_begin,
                    cb_begin + cb_count, c->ncb);
    int rc = ensure_workspace(c, false);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = dwt_forward_impl(c, d_frame, true, c->one.coef, s))) return rc;
    uint16_t *const st16 = reinterpret_cast<uint16_t *>(c->one.staging);
    if ((rc = bpc_encode_impl(c, c->one.coef, st16, c->one.sizes, s, cb_begin, cb_count))) return rc;
    return pack_range(c, st16 + (size_t)cb_begin * PICSONG_CB_WORDS, c->one.sizes + cb_begin, cb_count, nullptr,
                      d_stream, s);
}

// ---------------------------------------------------------------------------------------------
// batched frames: n frames of a video in ONE launch per stage (grid.z = frame for the DWT levels, n x the
// codeblock waves for the coder, grid.y = frame for the pack).  A 4K frame alone is 1020 coder waves -- one
// per SIMD, a quarter of what the coder needs to keep the vector pipes busy ("batch several
// frames per launch"); the reference's answer is -numberOfStreams worker threads with a stream each
// (Engines/CodingEngine.cu:990-1061), this is the same frames-in-flight idea without depending on the
// runtime's queues.
// ---------------------------------------------------------------------------------------------
static int ensure_batch(picsong_ctx *c, int n)
{
    if (n <= c->batch_cap) return PICSONG_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());                 // a smaller batch may still be running on the old buffers
    free_batch(c);
    // (scratch for whole workgroups per frame: the RGB form pads every component's waves to workgroups)
    const size_t waves = (size_t)n * (size_t)dec_scratch_waves(c);
    Workspace &w = c->batch;
    HIP_TRY(hipMalloc(&w.coef, (size_t)n * (c->P + c->extra) * 4));
    HIP_TRY(hipMalloc(&w.staging, (size_t)n * c->P * sizeof(int32_t)));
    HIP_TRY(hipMalloc(&w.sizes, (size_t)n * (size_t)c->ncb * sizeof(int32_t)));
    HIP_TRY(hipMalloc(&w.offsets, (size_t)n * (size_t)c->ncb * sizeof(int32_t)));
    HIP_TRY(hipMalloc(&w.total, (size_t)n * sizeof(int32_t)));
    HIP_TRY(hipMalloc(&w.plane_scratch, waves * kEncScratchDwordsPerWave * sizeof(uint32_t)));
    HIP_TRY(hipHostMalloc(&c->h_totals, (size_t)n * sizeof(int32_t)));
    c->batch_cap = n;
    return PICSONG_OK;
}

// n planes of P 32-bit words: the decoded coefficients of a batch / the colour-transformed components of an RGB frame
static int ensure_coef_i(picsong_ctx *c, int n)
{
    if (c->b_coef_i_cap >= n) return PICSONG_OK;
    HIP_TRY(hipDeviceSynchronize());
    if (c->batch.coef_i) (void)hipFree(c->batch.coef_i);
    c->batch.coef_i = nullptr; c->b_coef_i_cap = 0;
    HIP_TRY(hipMalloc(&c->batch.coef_i, (size_t)n * c->P * sizeof(int32_t)));
    c->b_coef_i_cap = n;
    return PICSONG_OK;
}

int picsong_encode_frames(picsong_ctx *c, int n, const uint8_t *d_frames, size_t frame_stride, int first_iter,
                          uint16_t *d_streams, size_t stream_stride, void *stream)
{
    REFUSE_DEEP(c, "encode_frames");
    if (!c || !d_frames || !d_streams) return fail(PICSONG_ERR_ARG, "encode_frames: null argument");
    if (n < 1 || n > 64) return fail(PICSONG_ERR_ARG, "encode_frames: %d frames outside 1..64", n);
    if (n > 1 && (frame_stride < c->P || stream_stride < picsong_max_stream_shorts(c->aw, c->ah)))
        return fail(PICSONG_ERR_ARG, "encode_frames: strides smaller than a padded frame / a worst-case codestream");
    if (c->p.cp == 3 || c->p.is_rgb)
        return fail(PICSONG_ERR_ARG, "encode_frames: grey -cp 2 contexts only (-cp 3 is coded frame by frame: picsong_encode_frame; "
                                     "an RGB frame's components: picsong_encode_rgb_frame)");
    if (((uintptr_t)d_frames | frame_stride) & 15u) return fail(PICSONG_ERR_ARG, "encode_frames: frames must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));                       // (a caller with several devices may be on another one)
    BpcArgs a;
    int rc = bpc_args(c, a, 0);
    if (rc) return rc;
    if ((rc = ensure_batch(c, n))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t coef_z = (c->P + c->extra) * 4;
    hipEvent_t *ev = nullptr;                             // stage timers: one set per batch (picsong_profile_begin)
    if (c->prof_cap > 0 && c->prof_n < c->prof_cap) ev = c->prof_ev->data() + 4 * (c->prof_n++);
    if (ev) HIP_TRY(hipEventRecord(ev[0], s));

    // ---- DWT: the single-frame plan of frame 0 with grid.z = n
    std::vector<FwdLaunch> plan = plan_dwt_forward(d_frames, true, c->batch.coef, c->aw, c->ah, c->p.wl, c->p.qs, c->c16);
    a.c16 = plan_is_c16(plan) ? 1 : 0;
    plan_frame_strides(plan, frame_stride, coef_z);
    if ((rc = launch_fwd_plan(HipGo{ s }, c->p.lossy != 0, plan, (unsigned)n))) return rc;

    if (ev) HIP_TRY(hipEventRecord(ev[1], s));
    // ---- coder: one grid over the n frames' codeblock pairs
    const int wpf = (c->ncb + 1) / 2;
    a.cb_base = 0; a.nCB = c->ncb;
    a.coeffs_in = c->batch.coef; a.is_float = c->p.lossy ? 1 : 0;
    a.staging16 = reinterpret_cast<uint16_t *>(c->batch.staging);   // (16-bit staging: frame f's at + f * P shorts)
    a.sizes = c->batch.sizes; a.plane_scratch = c->batch.plane_scratch;
    a.frames = n; a.waves_per_frame = wpf; a.coef_z = coef_z;
    // (-k > 0, one-wave workgroups: a frame is exactly its codeblock pairs, no padding waves)
    if ((rc = launch_encoder(c, a, (unsigned)n * (unsigned)wpf, 0, 1, s))) return rc;

    if (ev) HIP_TRY(hipEventRecord(ev[2], s));
    // ---- pack: the populated header where the batch holds the video's frame 0
    uint16_t hdr[PICSONG_HDR_SHORTS];
    const bool has0 = first_iter <= 0 && first_iter + n > 0;
    if (has0) picsong_header_pack(&c->p, hdr);
    if ((rc = pack_frames(HipGo{ s }, a.staging16, c->batch, c->ncb, (unsigned)n, has0 ? hdr : nullptr, -first_iter + 1, d_streams,
                          c->P, stream_stride))) return rc;
    if (ev) HIP_TRY(hipEventRecord(ev[3], s));
    c->last_batch = n;
    return PICSONG_OK;
}

int picsong_last_totals(picsong_ctx *c, void *stream, int n, int *h_totals)
{
    if (!c || !h_totals) return fail(PICSONG_ERR_ARG, "last_totals: null argument");
    if (n < 1 || n > c->last_batch) return fail(PICSONG_ERR_ARG, "last_totals: %d frames, the last batch had %d", n, c->last_batch);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(c->h_totals, c->batch.total, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < n; i++) h_totals[i] = c->h_totals[i];
    return PICSONG_OK;
}

// What the decode sequences (decode_frames and decode_rgb_frames, launch_seq.hpp) take from a context: its geometry and
// switches, the tables of `a` (grey: component 0's; rgb: the three, bpc_args_rgb)
static DecodeCtx decode_ctx(picsong_ctx *c, const BpcArgs &a, bool rgb)
{
    DecodeCtx g;
    g.aw = c->aw; g.ah = c->ah; g.wl = c->p.wl; g.ncb = c->ncb;
    g.lossy = c->p.lossy != 0; g.qs = c->p.qs; g.fast_div = c->fast_div; g.off = level_off(c);
    g.P = c->P; g.extra = c->extra;
    g.rgb = rgb; g.cp3 = c->p.cp == 3;
    g.direct = dec_from_stream(c);
    g.compact = a.k > 0.0f && bulk_compact(c, 0, rgb ? 3 : 1);
    g.max_stream = (uint32_t)picsong_max_stream_shorts(c->aw, c->ah);
    g.flag = c->d_flag;
    g.px_max = is_deep(c) ? px_max(c) : 0;               // (a deep context's decode calls are the *16 ones)
    return g;
}

// n grey frames decoded through ONE launch per stage (decode_frames, launch_seq.hpp): the mirror of picsong_encode_frames.
// n = 1: on the frame's own workspace, what the single-frame calls have always used (and picsong_last_total reads);
// n > 1: on the batch's.  The arguments have passed the caller's checks.
static int decode_grey(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, uint8_t *d_out, size_t frame_stride,
                       void *stream, int reduce, const WindowPlan *win = nullptr, size_t pitch = 0)
{
    int rc;
    if (n == 1) {
        if ((rc = ensure_workspace(c, true))) return rc;
        if ((rc = ensure_plane_scratch(c))) return rc;      // the decoder parks its finished planes there too
    } else {
        HIP_TRY(hipSetDevice(c->device));
        if ((rc = ensure_batch(c, n))) return rc;
        c->last_batch = -1;                                 // the batch buffers hold a decode now: no encode totals to hand out
        if ((rc = ensure_coef_i(c, n))) return rc;
    }
    BpcArgs a;
    if ((rc = bpc_args(c, a, 0))) return rc;
    // (16-bit coefficients between the decoder and the synthesis where the context's magnitudes are bounded and this
    // call's pointers take the vector kernels: dec_c16_reduced, plan_inv_is_c16)
    return refused_rc(decode_frames(HipGo{ (hipStream_t)stream }, decode_ctx(c, a, false), a, n == 1 ? c->one : c->batch, (unsigned)n,
                                    d_streams, stream_stride, reduce, win, dec_c16_reduced(c, reduce), lean97_levels(), d_out,
                                    frame_stride, pitch));
}

// picsong_decode_frames (reduce = 0) and picsong_decode_frames_reduced: frame f's pixels of level `reduce` at
// d_frames_out + f * frame_stride, row stride AW >> reduce
// win != nullptr (picsong_decode_frames_window): frame f's window of level `reduce` at d_frames_out + f * frame_stride,
// row stride pitch
static int decode_frames_impl(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, uint8_t *d_frames_out,
                              size_t frame_stride, void *stream, int reduce, const char *who,
                              const WindowPlan *win = nullptr, size_t pitch = 0)
{
    REFUSE_DEEP(c, who);
    if (!c || !d_streams || !d_frames_out) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    if (n < 1 || n > 64) return fail(PICSONG_ERR_ARG, "%s: n = %d outside 1..64", who, n);
    if (c->p.cp == 3 || c->p.is_rgb)
        return fail(PICSONG_ERR_ARG, "%s: grey -cp 2 contexts only (-cp 3: frame by frame; RGB: picsong_decode_rgb_frame)", who);
    if (!reduce_ok(c->p.wl, reduce))
        return fail(PICSONG_ERR_ARG, "%s: reduce %d outside 0..%d (wl - 1)", who, reduce, c->p.wl - 1);
    const size_t px = (size_t)(c->aw >> reduce) * (size_t)(c->ah >> reduce);      // bytes of one frame's pixels
    // (a window's bytes: its last row ends (h - 1) * pitch + w bytes in)
    const size_t span = win ? (size_t)(win->R[reduce].y1 - win->R[reduce].y0 - 1) * pitch + (size_t)(win->R[reduce].x1 - win->R[reduce].x0) : px;
    if (n > 1 && (stream_stride < picsong_max_stream_shorts(c->aw, c->ah) || frame_stride < span))
        return fail(PICSONG_ERR_ARG, "%s: strides %zu shorts / %zu bytes too small", who, stream_stride, frame_stride);
    return decode_grey(c, n, d_streams, stream_stride, d_frames_out, frame_stride, stream, reduce, win, pitch);
}

// The single-frame calls: the n = 1 case of the same sequence, on the frame's own workspace.  picsong_decode_frame takes
// what a context holds, -cp 3 through the staging included.
int picsong_decode_frame(picsong_ctx *c, const uint16_t *d_stream, uint8_t *d_frame_out, void *stream)
{
    REFUSE_DEEP(c, "decode_frame");
    if (!c || !d_frame_out || !d_stream) return fail(PICSONG_ERR_ARG, "decode_frame: null argument");
    return decode_grey(c, 1, d_stream, 0, d_frame_out, 0, stream, 0);
}

int picsong_decode_frame_reduced(picsong_ctx *c, const uint16_t *d_stream, int reduce, uint8_t *d_out, void *stream)
{
    REFUSE_DEEP(c, "decode_frame_reduced");
    if (!c || !d_out || !d_stream) return fail(PICSONG_ERR_ARG, "decode_frame_reduced: null argument");
    if (int rc = reduced_args_ok(c, reduce, "decode_frame_reduced")) return rc;
    return decode_grey(c, 1, d_stream, 0, d_out, 0, stream, reduce);
}

int picsong_decode_frame_window(picsong_ctx *c, const uint16_t *d_stream, int reduce, int x, int y, int w, int h,
                                uint8_t *d_out, size_t out_pitch, void *stream)
{
    REFUSE_DEEP(c, "decode_frame_window");
    if (!c || !d_out || !d_stream) return fail(PICSONG_ERR_ARG, "decode_frame_window: null argument");
    WindowPlan plan;
    if (int rc = window_args_ok(c, reduce, x, y, w, h, "decode_frame_window", &plan)) return rc;
    if (out_pitch < (size_t)w) return fail(PICSONG_ERR_ARG, "decode_frame_window: out_pitch %zu < w %d", out_pitch, w);
    return decode_grey(c, 1, d_stream, 0, d_out, 0, stream, reduce, &plan, out_pitch);
}

int picsong_decode_frames(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, uint8_t *d_frames_out,
                          size_t frame_stride, void *stream)
{
    return decode_frames_impl(c, n, d_streams, stream_stride, d_frames_out, frame_stride, stream, 0, "decode_frames");
}

int picsong_decode_frames_reduced(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, int reduce,
                                  uint8_t *d_frames_out, size_t frame_stride, void *stream)
{
    return decode_frames_impl(c, n, d_streams, stream_stride, d_frames_out, frame_stride, stream, reduce,
                              "decode_frames_reduced");
}

int picsong_decode_frames_window(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, int reduce, int x,
                                 int y, int w, int h, uint8_t *d_out, size_t out_pitch, size_t frame_stride, void *stream)
{
    REFUSE_DEEP(c, "decode_frames_window");
    const char *who = "decode_frames_window";
    if (!c || !d_streams || !d_out) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    WindowPlan plan;
    if (int rc = window_args_ok(c, reduce, x, y, w, h, who, &plan)) return rc;
    if (out_pitch < (size_t)w) return fail(PICSONG_ERR_ARG, "%s: out_pitch %zu < w %d", who, out_pitch, w);
    return decode_frames_impl(c, n, d_streams, stream_stride, d_out, frame_stride, stream, reduce, who, &plan, out_pitch);
}

int picsong_copy_last_totals(picsong_ctx *c, void *stream, int n, int32_t *d_totals)
{
    if (!c || !d_totals) return fail(PICSONG_ERR_ARG, "copy_last_totals: null argument");
    // last_batch = 0: the most recent call that packed a stream was a single-frame one (picsong_encode_frame, a stripe,
    // a plane, picsong_bitstream_pack: every writer of d_total resets it); -1: a batched decode has used the buffers
    const bool single = n == 1 && c->last_batch == 0;
    if (!single && (n < 1 || n > c->last_batch))
        return fail(PICSONG_ERR_ARG, "copy_last_totals: %d frames, the last batch had %d", n, c->last_batch);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(d_totals, single ? c->one.total : c->batch.total, (size_t)n * sizeof(int32_t),
                           hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PICSONG_OK;
}

// ---------------------------------------------------------------------------------------------
// deep contexts (bit_depth 9..16): uint16 samples at the transform's two ends, everything between as ever (32-bit
// coefficient arrays, no fused head or tail).  PICSONG_DEEP_NOFUSE=1 (read per call): the element-wise passes.
// ---------------------------------------------------------------------------------------------
int picsong_depth_range_guaranteed(int bit_depth, int lossy, int wl, float qs, int *yes)
{
    if (!yes) return fail(PICSONG_ERR_ARG, "depth_range_guaranteed: null argument");
    if (bit_depth < 8 || bit_depth > 16) return fail(PICSONG_ERR_ARG, "depth_range_guaranteed: bit depth %d outside 8..16", bit_depth);
    if (wl < 1 || wl > 7) return fail(PICSONG_ERR_ARG, "depth_range_guaranteed: wl %d outside 1..7", wl);
    if (lossy && !(qs > 0.0f && qs <= 1.0f)) return fail(PICSONG_ERR_ARG, "depth_range_guaranteed: qs %g outside (0,1]", qs);
    *yes = coef16_bound(lossy != 0, wl, qs, 1 << (bit_depth - 1)) ? 1 : 0;
    return PICSONG_OK;
}

// ... of a deep RGB context: the RCT's chroma differences span +-(2^bd - 1), one bit more than a grey sample; the ICT's rows
// have absolute sum 1, so its components stay within +-2^(bd-1)
int picsong_depth_range_guaranteed_rgb(int bit_depth, int lossy, int wl, float qs, int *yes)
{
    if (!yes) return fail(PICSONG_ERR_ARG, "depth_range_guaranteed_rgb: null argument");
    if (bit_depth < 9 || bit_depth > 16) return fail(PICSONG_ERR_ARG, "depth_range_guaranteed_rgb: bit depth %d outside 9..16", bit_depth);
    if (wl < 1 || wl > 7) return fail(PICSONG_ERR_ARG, "depth_range_guaranteed_rgb: wl %d outside 1..7", wl);
    if (lossy && !(qs > 0.0f && qs <= 1.0f)) return fail(PICSONG_ERR_ARG, "depth_range_guaranteed_rgb: qs %g outside (0,1]", qs);
    *yes = coef16_bound(lossy != 0, wl, qs, lossy ? 1 << (bit_depth - 1) : 1 << bit_depth) ? 1 : 0;
    return PICSONG_OK;
}

int picsong_level_shift_fwd16(picsong_ctx *c, const uint16_t *d_in, void *d_out, void *stream)
{
    REFUSE_SHALLOW(c, "level_shift_fwd16");
    if (!c || !d_in || !d_out) return fail(PICSONG_ERR_ARG, "level_shift_fwd16: null argument");
    if (((uintptr_t)d_in) & 1u) return fail(PICSONG_ERR_ARG, "level_shift_fwd16: uint16 samples need a 2-byte aligned pointer");
    return level_shift_fwd16(HipGo{ (hipStream_t)stream }, c->p.lossy != 0, d_in, d_out, c->P / 4, level_off(c));
}

int picsong_dwt_forward_u16(picsong_ctx *c, const uint16_t *d_in, void *d_out, void *stream)
{
    REFUSE_SHALLOW(c, "dwt_forward_u16");
    if (!c || !d_in || !d_out) return fail(PICSONG_ERR_ARG, "dwt_forward_u16: null argument");
    if (((uintptr_t)d_in) & 1u) return fail(PICSONG_ERR_ARG, "dwt_forward_u16: uint16 samples need a 2-byte aligned pointer");
    const bool nofuse = deep_nofuse();
    if (nofuse) if (int rc = ensure_workspace(c, false)) return rc;      // (the shifted samples: the frame's staging)
    return deep_forward(HipGo{ (hipStream_t)stream }, c->p.lossy != 0, nofuse, d_in, 0, 1u, d_out, c->one.staging, c->aw, c->ah, c->p.wl,
                        c->p.qs, level_off(c), 0);
}

// what the two frame calls refuse alike (nothing launched)
static int frames16_args_ok(const picsong_ctx *c, int n, const void *d_frames, size_t frame_stride, const void *d_streams,
                            size_t stream_stride, const char *who)
{
    REFUSE_SHALLOW(c, who);
    if (c && is_deep_rgb(c))
        return fail(PICSONG_ERR_ARG, "%s: grey frames on an RGB context (its frame calls: picsong_encode_rgb_frames16, "
                                     "picsong_decode_rgb_frames16)", who);
    if (!c || !d_frames || !d_streams) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    if (n < 1 || n > 64) return fail(PICSONG_ERR_ARG, "%s: %d frames outside 1..64", who, n);
    if (c->p.cp == 3) return fail(PICSONG_ERR_ARG, "%s: -cp 2 contexts only", who);
    if ((((uintptr_t)d_frames) | ((uintptr_t)d_streams)) & 1u) return fail(PICSONG_ERR_ARG, "%s: pointers need 2-byte alignment", who);
    if (n > 1 && ((frame_stride & 1u) || frame_stride < 2 * c->P))
        return fail(PICSONG_ERR_ARG, "%s: frame_stride %zu must be even and at least a padded frame's %zu bytes", who, frame_stride, 2 * c->P);
    if (n > 1 && stream_stride < picsong_max_stream_shorts(c->aw, c->ah))
        return fail(PICSONG_ERR_ARG, "%s: stream stride smaller than a worst-case codestream", who);
    return PICSONG_OK;
}

int picsong_encode_frames16(picsong_ctx *c, int n, const uint16_t *d_frames, size_t frame_stride, int first_iter,
                            uint16_t *d_streams, size_t stream_stride, void *stream)
{
    int rc = frames16_args_ok(c, n, d_frames, frame_stride, d_streams, stream_stride, "encode_frames16");
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    BpcArgs a;
    if ((rc = bpc_args(c, a, 0))) return rc;
    if ((rc = ensure_batch(c, n))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t coef_z = (c->P + c->extra) * 4;
    // ---- DWT: level 0 reads the uint16 samples (grid.z = n); the batch's staging holds the shifted samples of the
    // element-wise route until the coder overwrites it
    if ((rc = deep_forward(HipGo{ s }, c->p.lossy != 0, deep_nofuse(), d_frames, frame_stride, (unsigned)n, c->batch.coef, c->batch.staging,
                           c->aw, c->ah, c->p.wl, c->p.qs, level_off(c), coef_z))) return rc;
    // ---- coder: one grid over the n frames' codeblock pairs, 32-bit coefficients
    const int wpf = (c->ncb + 1) / 2;
    a.c16 = 0;
    a.cb_base = 0; a.nCB = c->ncb;
    a.coeffs_in = c->batch.coef; a.is_float = c->p.lossy ? 1 : 0;
    a.staging16 = reinterpret_cast<uint16_t *>(c->batch.staging);
    a.sizes = c->batch.sizes; a.plane_scratch = c->batch.plane_scratch;
    a.frames = n; a.waves_per_frame = wpf; a.coef_z = coef_z;
    if ((rc = launch_encoder(c, a, (unsigned)n * (unsigned)wpf, 0, 1, s))) return rc;
    // ---- pack: the populated header (both depth fields carry bit_depth) where the batch holds the video's frame 0
    uint16_t hdr[PICSONG_HDR_SHORTS];
    const bool has0 = first_iter <= 0 && first_iter + n > 0;
    if (has0) picsong_header_pack(&c->p, hdr);
    if ((rc = pack_frames(HipGo{ s }, a.staging16, c->batch, c->ncb, (unsigned)n, has0 ? hdr : nullptr, -first_iter + 1, d_streams,
                          c->P, stream_stride))) return rc;
    c->last_batch = n;
    return PICSONG_OK;
}

int picsong_decode_frames16(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, uint16_t *d_frames_out,
                            size_t frame_stride, void *stream)
{
    if (int rc = frames16_args_ok(c, n, d_frames_out, frame_stride, d_streams, stream_stride, "decode_frames16")) return rc;
    // (decode_ctx hands the sequence px_max: uint16 samples at d_frames_out, frame_stride bytes apart)
    return decode_grey(c, n, d_streams, stream_stride, reinterpret_cast<uint8_t *>(d_frames_out), frame_stride, stream, 0);
}

// The proxies of deep grey frames: picsong_decode_frames_reduced / _window on uint16 samples, strides and pitch in bytes.
// The same sequence (decode_frames with DecodeCtx::px_max): the reduced corner's or the cone's codeblocks, the synthesis to
// level `reduce`, whose launch stores the clamped samples (reduced: where the output is 16-byte aligned and
// PICSONG_DEEP_NOFUSE is unset, else a clamp_pixels16 pass a frame; window: always).
int picsong_decode_frames16_reduced(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, int reduce,
                                    uint16_t *d_frames_out, size_t frame_stride, void *stream)
{
    const char *who = "decode_frames16_reduced";
    if (!c) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    if (const char *why = frames16_reduced_refusal(c->p.bit_depth, c->p.is_rgb != 0, c->p.cp, n, d_frames_out, d_streams, frame_stride, stream_stride,
                                                   picsong_max_stream_shorts(c->aw, c->ah), c->aw, c->ah, c->p.wl, reduce))
        return fail(PICSONG_ERR_ARG, "%s: %s", who, why);
    return decode_grey(c, n, d_streams, stream_stride, reinterpret_cast<uint8_t *>(d_frames_out), frame_stride, stream, reduce);
}

int picsong_decode_frames16_window(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, int reduce, int x, int y, int w,
                                   int h, uint16_t *d_out, size_t out_pitch, size_t frame_stride, void *stream)
{
    const char *who = "decode_frames16_window";
    if (!c) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    if (const char *why = frames16_window_refusal(c->p.bit_depth, c->p.is_rgb != 0, c->p.cp, n, d_out, d_streams, out_pitch, frame_stride,
                                                  stream_stride, picsong_max_stream_shorts(c->aw, c->ah), c->aw, c->ah, c->p.wl, reduce, x, y,
                                                  w, h))
        return fail(PICSONG_ERR_ARG, "%s: %s", who, why);
    WindowPlan plan;
    if (int rc = window_args_ok(c, reduce, x, y, w, h, who, &plan)) return rc;
    return decode_grey(c, n, d_streams, stream_stride, reinterpret_cast<uint8_t *>(d_out), frame_stride, stream, reduce, &plan, out_pitch);
}

// ---------------------------------------------------------------------------------------------
// RGB path
// ---------------------------------------------------------------------------------------------
int picsong_rgb_forward(picsong_ctx *c, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b, void *d_c0,
                        void *d_c1, void *d_c2, void *stream)
{
    REFUSE_DEEP(c, "rgb_forward");
    if (!c || !d_r || !d_g || !d_b || !d_c0 || !d_c1 || !d_c2) return fail(PICSONG_ERR_ARG, "rgb_forward: null argument");
    return rgb_forward(HipGo{ (hipStream_t)stream }, c->p.lossy != 0, d_r, d_g, d_b, d_c0, d_c1, d_c2, c->P / 4, level_off(c));
}

int picsong_rgb_inverse(picsong_ctx *c, const void *d_c0, const void *d_c1, const void *d_c2, uint8_t *d_r,
                        uint8_t *d_g, uint8_t *d_b, void *stream)
{
    REFUSE_DEEP(c, "rgb_inverse");
    if (!c || !d_r || !d_g || !d_b || !d_c0 || !d_c1 || !d_c2) return fail(PICSONG_ERR_ARG, "rgb_inverse: null argument");
    return rgb_inverse(HipGo{ (hipStream_t)stream }, c->p.lossy != 0, d_c0, d_c1, d_c2, d_r, d_g, d_b, c->P / 4, level_off(c));
}

int picsong_encode_plane(picsong_ctx *c, const void *d_plane, int comp, int with_header, uint16_t *d_stream, void *stream)
{
    if (!c || !d_plane || !d_stream) return fail(PICSONG_ERR_ARG, "encode_plane: null argument");
    int rc = ensure_workspace(c, false);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = dwt_forward_impl(c, d_plane, false, c->one.coef, s))) return rc;
    uint16_t *const st16 = reinterpret_cast<uint16_t *>(c->one.staging);
    if ((rc = bpc_encode_impl(c, c->one.coef, st16, c->one.sizes, s, 0, -1, comp))) return rc;
    uint16_t hdr[PICSONG_HDR_SHORTS];
    if (with_header) picsong_header_pack(&c->p, hdr);
    return pack_range(c, st16, c->one.sizes, c->ncb, with_header ? hdr : nullptr, d_stream, s);
}

int picsong_decode_plane(picsong_ctx *c, const uint16_t *d_stream, int comp, void *d_plane_out, void *stream)
{
    if (!c || !d_plane_out || !d_stream) return fail(PICSONG_ERR_ARG, "decode_plane: null argument");
    int rc = ensure_workspace(c, true);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    // (the stream's intake, then the coder -- reading the stream itself, or the staging)
    const bool direct = dec_from_stream(c);
    if ((rc = stream_intake(c, d_stream, 1u, 0, direct, c->one, s))) return rc;
    if ((rc = bpc_decode_impl(c, c->one.staging, c->one.sizes, c->one.coef_i, s, comp, direct ? d_stream : nullptr))) return rc;
    return picsong_dwt_inverse(c, c->one.coef_i, d_plane_out, stream);
}


// The three component tables of an RGB context for ONE coder grid: same geometry, every frame f of the batched
// launch coding with table f; k = 0: a component's waves_per_frame are whole workgroups; -k > 0 (one-wave workgroups):
// exactly its waves.
static int rgb_component_waves(const BpcArgs &a, int wpf) { return picsong::rgb_component_waves(a.k > 0.0f, wpf); }
static int bpc_args_rgb(picsong_ctx *c, BpcArgs &a)
{
    int rc = bpc_args(c, a, 0);
    if (rc) return rc;
    for (int k = 1; k < 3; k++) {
        if (!c->has_lut[k]) return fail(PICSONG_ERR_ARG, "no LUT loaded for component %d", k);
        const picsong_lut_info &x = c->li[0], &y = c->li[k];
        if (x.n_bitplanes != y.n_bitplanes || x.n_subbands != y.n_subbands || x.precision != y.precision ||
            x.n_ref != y.n_ref || x.n_sig != y.n_sig || x.n_sign != y.n_sign || x.n_tables != y.n_tables)
            return fail(PICSONG_ERR_ARG, "the components' tables differ in geometry: code the planes one by one (picsong_encode_plane)");
    }
    for (int k = 0; k < 3; k++) { a.lut_c[k] = c->d_lut[k]; a.img_c[k] = ctx_uses_plane_img(c) ? c->d_img[k] : nullptr; }
    a.cb_base = 0; a.nCB = c->ncb;
    a.frames = 3; a.waves_per_frame = rgb_component_waves(a, (c->ncb + 1) / 2);
    return PICSONG_OK;
}

// The colour transform and the forward transform of n RGB frames' 3 n components (rgb_forward_transform, launch_seq.hpp),
// plane z's coefficients into c->batch.coef + z * (P + extra) * 4 bytes (ensure_batch(3 n) and ensure_coef_i(3 n) done);
// *c16: the coefficient form this call's plan delivers.  The head of picsong_encode_rgb_frames and picsong_train_rgb_frame.
// (the fused head's buffer loads want all three planes, and every frame's with them, 16-byte aligned like a grey frame's)
static bool rgb_planes_aligned(const uint8_t *r, const uint8_t *g, const uint8_t *b) { return ((((uintptr_t)r) | ((uintptr_t)g) | ((uintptr_t)b)) & 15u) == 0; }
static int rgb_forward_transform(picsong_ctx *c, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b, hipStream_t s,
                                 bool *c16, int n = 1, size_t frame_stride = 0)
{
    const bool lossy = c->p.lossy != 0;
    const bool fuse = c->c16 && rgb_planes_aligned(d_r, d_g, d_b) && (n == 1 || (frame_stride & 15u) == 0) && !getenv("PICSONG_RGB_NOFUSE");
    auto plan_of = [c](const void *src, bool u8in) { return plan_dwt_forward(src, u8in, c->batch.coef, c->aw, c->ah, c->p.wl, c->p.qs, c->c16); };
    return picsong::rgb_forward_transform(HipGo{ s }, lossy, fuse, plan_of, true, d_r, d_g, d_b, c->batch.coef_i, c->P, level_off(c),
                                          (c->P + c->extra) * 4, c16, nullptr, (unsigned)n, frame_stride);
}

// ---------------------------------------------------------------------------------------------
// rate calls (encode to a target size) and quality calls (encode to a target distortion): ONE driver, search_impl, over
// rate_search.hpp's grid and walk (bisect_walk); rate_kernels.hpp: the quantise pass; quality_kernels.hpp: sse_kernel;
// launch_seq.hpp: frames_sse and quality_probe, the sequences the emulator driver of the tests runs too
//   1. the UNQUANTISED (unit-step) transform of the n frames (plan_dwt_forward_unit), once, into float Mallat arrays
//      (rate_transform);
//   2. per round of the search, the round's K candidates are measured and ONE read-back through pinned memory brings
//      their figures to the stepper:
//      size:    quantise_kernel writes the candidates' coefficients as K * n "frames" of the batch buffers, ONE batched
//               coder launch codes them, the size scan totals them -- no pack (rate_probe);
//      quality: quality_probe for each candidate, back to back over ONE set of nf-frame buffers (batch.coef_i,
//               batch.coef, and q_pix where the RGB probe's tail is the unfused one), candidate i's sums in slots
//               i * nf .. of d_sse.  No coder launch;
//   3. the winner is packed with a header whose qs field is the result (rate_finish): a size search packs it from the
//      last round's staging when it was coded there, else, as a quality search always, after one more quantise + coder
//      launch of it alone (rate_probe).
// PICSONG_RATE_K=1 keeps one candidate a round in both kinds (the measurements of tools/rate_bench.py compare both).
// RGB: nf = 3 n planes, plane 3 f + k component k of frame f.  The single-frame calls (n = 1) keep one candidate a
// size round; the n-frame calls (RateJob::multi) take rgb_search_candidates (rate_search.hpp).
// PICSONG_RGB_SSE_FUSED=0, read per call, keeps the RGB probe's unfused tail (rgb_inverse + frames_sse).
// The SSIM calls (kSearchSsim) are quality searches whose probe ends in ssim_kernel (frames_dssim) and whose figures are
// DSSIM sums; an RGB probe of theirs always takes the unfused tail.
// ---------------------------------------------------------------------------------------------
struct RateJob {
    int n;                                  // frames (RGB: three components each)
    const uint8_t *frames; size_t frame_stride;
    const uint8_t *r, *g, *b;               // RGB planes of frame 0 (frames == nullptr), frame f's frame_stride bytes behind
    int first_iter, header_mask;
    uint16_t *d_streams; size_t stream_stride;
    bool single;                            // picsong_encode_frame_rate: the length also where picsong_encode_frame leaves it
    bool multi = false;                     // the n-frame RGB calls (picsong_encode_rgb_frames_rate / _quality)
};

enum SearchKind { kSearchSize, kSearchQuality, kSearchSsim };   // (kSearchSsim: a quality search whose measure is the DSSIM sum)

static int search_candidates(const picsong_ctx *c, SearchKind kind, const RateJob &job)
{
    const char *e = getenv("PICSONG_RATE_K");
    const bool one = e && atoi(e) == 1;
    if (job.multi) return rgb_search_candidates(kind == kSearchSize, job.n, one);
    // the single-frame RGB calls' size search codes one candidate a round, as it always has (a quality search's probes
    // launch no coder)
    if (kind == kSearchSize && c->p.is_rgb) return 1;
    return one ? 1 : kRateMaxK;
}

static int ensure_rate(picsong_ctx *c, int frames)
{
    if (frames <= c->rate_cap) return PICSONG_OK;
    HIP_TRY(hipDeviceSynchronize());
    if (c->rate_coef) (void)hipFree(c->rate_coef);
    c->rate_coef = nullptr; c->rate_cap = 0;
    c->rate_z = ((c->P + c->extra + 3) & ~(size_t)3) * 4;   // (16-byte aligned arrays: quantise_kernel's loads)
    HIP_TRY(hipMalloc(&c->rate_coef, (size_t)frames * c->rate_z));
    c->rate_cap = frames;
    return PICSONG_OK;
}

// step 1: the unquantised coefficients of the job's frames (RGB: of the three components), array f at rate_coef + f * rate_z
static int rate_transform(picsong_ctx *c, const RateJob &job, hipStream_t s)
{
    const bool lossy = c->p.lossy != 0;
    if (!c->p.is_rgb) {
        std::vector<FwdLaunch> plan = plan_dwt_forward_unit(job.frames, true, c->rate_coef, c->aw, c->ah, c->p.wl);
        plan_frame_strides(plan, job.frame_stride, c->rate_z);
        return launch_fwd_plan(HipGo{ s }, lossy, plan, (unsigned)job.n);
    }
    // the ICT in the fused head's load stage where the planes allow it (as rgb_forward_transform), 32-bit float form
    auto plan_of = [c](const void *src, bool u8in) { return plan_dwt_forward_unit(src, u8in, c->rate_coef, c->aw, c->ah, c->p.wl); };
    const bool fuse = rgb_planes_aligned(job.r, job.g, job.b) && (job.n == 1 || (job.frame_stride & 15u) == 0) && !getenv("PICSONG_RGB_NOFUSE");
    return picsong::rgb_forward_transform(HipGo{ s }, lossy, fuse, plan_of, false, job.r, job.g, job.b, c->batch.coef_i, c->P, level_off(c),
                                          c->rate_z, nullptr, nullptr, (unsigned)job.n, job.frame_stride);
}

// step 2's launches for the candidates js[0 .. m): quantise, coder, size scan; the m * nf totals are then in batch.total
// (nf: coded arrays a candidate -- the n frames, or the 3 n components of n RGB frames; candidate i's plane z is plane
// i * nf + z of the launch, and nf a multiple of 3 keeps it on table z % 3)
static int rate_probe(picsong_ctx *c, BpcArgs a, int nf, int m, const int *js, hipStream_t s)
{
    int rc;
    const int in_max = c->p.is_rgb ? 255 : 128;
    bool c16 = c->p.bit_depth == 8 && dwt_c16_geometry_ok(c->aw, c->ah, c->p.wl);
    for (int i = 0; i < m; i++) c16 = c16 && coef16_ok(true, c->p.wl, rate_q(js[i]), in_max);
    const bool forms[kQuantMaxK] = { c16, c16, c16 };       // (one coder launch reads one form)
    const unsigned long long dst_z = (unsigned long long)c->P * 4ull;
    const QuantArgs qa = quantise_args(c->rate_coef, c->rate_z, c->batch.coef, dst_z, c->aw, c->ah, c->p.wl, nf, m, js, forms);
    const QuantLaunch ql = select_quantise(m, nf, c->ah);
    if ((rc = HipGo{ s }(ql.kernel, dim3(ql.wgs), 256u, qa))) return rc;
    a.c16 = c16 ? 1 : 0; a.is_float = 1;
    a.coeffs_in = c->batch.coef; a.coef_z = dst_z;
    a.staging16 = reinterpret_cast<uint16_t *>(c->batch.staging);
    a.sizes = c->batch.sizes; a.plane_scratch = c->batch.plane_scratch;
    if (c->p.is_rgb) {                                      // (plane z codes with table z % 3; waves_per_frame: bpc_args_rgb's)
        a.frames = m * nf;
        if ((rc = launch_encoder(c, a, (unsigned)(m * nf) * (unsigned)a.waves_per_frame, 0, 3, s))) return rc;
    } else {
        a.cb_base = 0; a.nCB = c->ncb;
        a.frames = m * nf; a.waves_per_frame = (c->ncb + 1) / 2;
        if ((rc = launch_encoder(c, a, (unsigned)(m * nf) * (unsigned)a.waves_per_frame, 0, 1, s))) return rc;
    }
    return HipGo{ s }(scan_sizes_kernel, dim3((unsigned)(m * nf)), scan_threads(c->ncb), c->batch.sizes, c->ncb, c->batch.offsets, c->batch.total);
}

// step 3: the pack of the result j, coded as candidate `slot` of the batch buffers by rate_probe, with its gain in the
// header; the lengths to h_totals and where the plain calls leave theirs.  Synchronises the stream.
static int rate_finish(picsong_ctx *c, const RateJob &job, int nf, int j, int slot, hipStream_t s, int *h_totals)
{
    int rc;
    const bool rgb = c->p.is_rgb != 0;
    Workspace w = c->batch;
    w.sizes += (size_t)slot * (size_t)nf * (size_t)c->ncb; w.offsets += (size_t)slot * (size_t)nf * (size_t)c->ncb;
    w.total += (size_t)slot * (size_t)nf;
    const uint16_t *st16 = reinterpret_cast<const uint16_t *>(c->batch.staging) + (size_t)slot * (size_t)nf * c->P;
    picsong_params hp = c->p;
    hp.qs = rate_q(j);
    uint16_t hdr[PICSONG_HDR_SHORTS];
    picsong_header_pack(&hp, hdr);
    if (rgb) {
        if ((rc = pack_rgb_frames(HipGo{ s }, st16, w, c->ncb, (unsigned)job.n, hdr, job.first_iter, job.header_mask, job.d_streams, c->P,
                                  job.stream_stride))) return rc;
    } else {
        const bool has_hdr = job.first_iter <= 0 && job.first_iter + job.n > 0;
        if ((rc = pack_frames(HipGo{ s }, st16, w, c->ncb, (unsigned)nf, has_hdr ? hdr : nullptr, -job.first_iter + 1, job.d_streams, c->P,
                              job.stream_stride))) return rc;
    }
    // (the lengths where the plain calls leave theirs: picsong_last_total(s) / picsong_copy_last_totals cover a rate call)
    if (slot > 0) HIP_TRY(hipMemcpyAsync(c->batch.total, w.total, (size_t)nf * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (job.single) HIP_TRY(hipMemcpyAsync(c->one.total, w.total, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->h_totals, w.total, (size_t)nf * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int f = 0; f < nf; f++) h_totals[f] = c->h_totals[f];
    c->last_batch = job.single ? 0 : nf;
    return PICSONG_OK;
}

// ---- the quality calls' conversions, picsong_frames_sse and probe buffers
constexpr int kQualitySlots = kRateMaxK * 3 * kRgbMaxFrames;   // (K candidates of 21 RGB frames' planes; 16 grey frames fit)

int picsong_psnr_to_sse(double psnr_db, uint64_t samples, uint64_t *max_sse)
{
    if (!max_sse) return fail(PICSONG_ERR_ARG, "psnr_to_sse: null argument");
    if (samples == 0) return fail(PICSONG_ERR_ARG, "psnr_to_sse: no samples");
    if (!std::isfinite(psnr_db)) return fail(PICSONG_ERR_ARG, "psnr_to_sse: the PSNR must be finite");
    const double v = std::floor(65025.0 * (double)samples / std::pow(10.0, psnr_db / 10.0));
    *max_sse = v >= 18446744073709551615.0 ? UINT64_MAX : (uint64_t)v;
    return PICSONG_OK;
}

int picsong_sse_to_psnr(uint64_t sse, uint64_t samples, double *psnr_db)
{
    if (!psnr_db) return fail(PICSONG_ERR_ARG, "sse_to_psnr: null argument");
    if (samples == 0) return fail(PICSONG_ERR_ARG, "sse_to_psnr: no samples");
    *psnr_db = sse == 0 ? HUGE_VAL : 10.0 * std::log10(65025.0 * (double)samples / (double)sse);
    return PICSONG_OK;
}

int picsong_frames_sse(picsong_ctx *c, int n, const uint8_t *d_a, size_t a_stride, const uint8_t *d_b, size_t b_stride,
                       uint64_t *d_sse, void *stream)
{
    REFUSE_DEEP(c, "frames_sse");
    if (!c || !d_a || !d_b || !d_sse) return fail(PICSONG_ERR_ARG, "frames_sse: null argument");
    if (n < 1 || n > kSseMaxFrames) return fail(PICSONG_ERR_ARG, "frames_sse: %d frames outside 1..%d", n, kSseMaxFrames);
    if (n > 1 && (a_stride < c->P || b_stride < c->P)) return fail(PICSONG_ERR_ARG, "frames_sse: strides smaller than a padded frame");
    HIP_TRY(hipSetDevice(c->device));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the kernel's sums are the interface's");
    return frames_sse(HipGo{ (hipStream_t)stream }, d_a, (size_t)c->aw, n > 1 ? a_stride : 0, d_b, (size_t)c->aw, n > 1 ? b_stride : 0,
                      c->p.width, c->p.height, n, reinterpret_cast<unsigned long long *>(d_sse));
}

// frames: the planes of probe pixels (q_pix) the call needs -- 0 for an RGB probe on the fused tail, which writes none
static int ensure_quality(picsong_ctx *c, int frames)
{
    if (!c->d_sse) HIP_TRY(hipMalloc(&c->d_sse, kQualitySlots * sizeof(unsigned long long)));
    if (!c->h_sse) HIP_TRY(hipHostMalloc(&c->h_sse, kQualitySlots * sizeof(unsigned long long)));
    if (frames <= c->q_cap) return PICSONG_OK;
    HIP_TRY(hipDeviceSynchronize());
    if (c->q_pix) (void)hipFree(c->q_pix);
    c->q_pix = nullptr; c->q_cap = 0;
    HIP_TRY(hipMalloc(&c->q_pix, (size_t)frames * c->P));
    c->q_cap = frames;
    return PICSONG_OK;
}

static int search_impl(picsong_ctx *c, const RateJob &job, SearchKind kind, uint64_t limit, int j_min, int j_max, hipStream_t s,
                       int *h_j, int *h_totals, uint64_t *h_sse, const char *who)
{
    // (search_args_ok has made the null, context-kind, stride and alignment checks)
    const bool size = kind == kSearchSize, ssim = kind == kSearchSsim;
    if (!c->p.lossy) return fail(PICSONG_ERR_ARG, "%s: a lossless context has no quantiser to search", who);
    if (c->p.cp == 3) return fail(PICSONG_ERR_ARG, "%s: -cp 3 contexts have no %s control", who, size ? "rate" : (ssim ? "SSIM" : "quality"));
    if (ssim && !ssim_geometry_ok(c->p.width, c->p.height)) return fail(PICSONG_ERR_ARG, "%s: the SSIM's 8 x 8 windows need a frame of 8 x 8 or more", who);
    if (size && limit == 0) return fail(PICSONG_ERR_ARG, "%s: target_shorts must be positive", who);
    if (!rate_range_ok(j_min, j_max))
        return fail(PICSONG_ERR_ARG, "%s: range [%d, %d] is neither 0, 0 (the whole grid) nor inside 1..%d", who, j_min, j_max, kRateJMax);
    const std::vector<int> grid = rate_grid(j_min, j_max);
    if (grid.empty()) return fail(PICSONG_ERR_ARG, "%s: no header-exact quantiser in [%d, %d]", who, j_min, j_max);
    HIP_TRY(hipSetDevice(c->device));
    const bool rgb = c->p.is_rgb != 0;
    const int nf = rgb ? 3 * job.n : job.n, K = search_candidates(c, kind, job);
    BpcArgs a;
    int rc = rgb ? bpc_args_rgb(c, a) : bpc_args(c, a, 0);   // (the encodes' table: refused before anything is launched)
    if (rc) return rc;
    // (a size round codes K candidates; a quality round measures them one after the other over nf-frame buffers)
    if ((rc = ensure_batch(c, size ? K * nf : nf))) return rc;
    if ((rgb || !size) && (rc = ensure_coef_i(c, nf))) return rc;
    if ((rc = ensure_rate(c, nf))) return rc;
    // (the probe of every round: PICSONG_RGB_SSE_FUSED and the buffers' alignment are the call's, not the round's)
    const char *const fe = getenv("PICSONG_RGB_SSE_FUSED");
    QualityProbe probe = { c->rate_coef, (unsigned long long)c->rate_z, c->batch.coef_i, c->batch.coef, nullptr,
                           c->aw, c->ah, c->p.wl, c->p.width, c->p.height, level_off(c), c->P, c->extra, nf,
                           job.frames, job.frame_stride, job.r, job.g, job.b, !(fe && atoi(fe) == 0), ssim };
    if (!size) {
        if ((rc = ensure_quality(c, quality_probe_fuses(probe) ? 0 : nf))) return rc;
        probe.pix = c->q_pix;
    }
    c->last_batch = -1;                                     // (until the result is packed: no totals to hand out)
    if ((rc = rate_transform(c, job, s))) return rc;

    // A round's measure: the launches of its m candidates, ONE read-back, ONE synchronise; values[i] = candidate i's total.
    // Size: one launch sequence codes all m (rate_probe).
    auto measure_size = [&](int m, const int *js, uint64_t *values) -> int {
        if (int e = rate_probe(c, a, nf, m, js, s)) return e;
        HIP_TRY(hipMemcpyAsync(c->h_totals, c->batch.total, (size_t)(m * nf) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int i = 0; i < m; i++)
            for (int f = 0; f < nf; f++) values[i] += (uint64_t)c->h_totals[i * nf + f];
        return PICSONG_OK;
    };
    // Quality: quality_probe per candidate, back to back; every probe made is kept with its per-array sums for h_sse.
    std::vector<int> seen_j;
    std::vector<uint64_t> seen_sse;
    auto measure_quality = [&](int m, const int *js, uint64_t *values) -> int {
        for (int i = 0; i < m; i++) {
            // stage timers (picsong_profile_begin): a probe records quantise, synthesis and SSE where a frame records
            // transform, coder and pack
            hipEvent_t *ev = nullptr;
            if (c->prof_cap > 0 && c->prof_n < c->prof_cap) ev = c->prof_ev->data() + 4 * (c->prof_n++);
            if (ev) HIP_TRY(hipEventRecord(ev[0], s));
            auto mark = [ev, s](int k) -> int {
                if (ev) HIP_TRY(hipEventRecord(ev[k], s));
                return PICSONG_OK;
            };
            if (int e = quality_probe(HipGo{ s }, probe, js[i], c->d_sse + i * nf, mark)) return e;
        }
        HIP_TRY(hipMemcpyAsync(c->h_sse, c->d_sse, (size_t)(m * nf) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int i = 0; i < m; i++) {
            seen_j.push_back(js[i]);
            for (int f = 0; f < nf; f++) { values[i] += c->h_sse[i * nf + f]; seen_sse.push_back(c->h_sse[i * nf + f]); }
        }
        return PICSONG_OK;
    };
    const BisectWalk w = size ? bisect_walk(grid, limit, K, Bisect::Largest, measure_size)
                              : bisect_walk(grid, limit, K, Bisect::Smallest, measure_quality);
    if (w.rc) return w.rc;
    *h_j = 0;
    if (w.result < 0)
        return size ? fail(PICSONG_ERR_RATE, "%s: no quantiser of the search range meets %llu shorts", who, (unsigned long long)limit)
                    : fail(PICSONG_ERR_QUALITY, "%s: no quantiser of the search range meets %s of %llu", who, ssim ? "a DSSIM sum" : "an SSE",
                           (unsigned long long)limit);
    const int j = grid[(size_t)w.result];
    // ---- the winner's staging: candidate `slot` of a size search's last round, or coded once more on its own
    int slot = -1;
    if (size) for (int i = 0; i < w.m; i++) if (w.js[i] == j) slot = i;
    if (slot < 0) {
        if ((rc = rate_probe(c, a, nf, 1, &j, s))) return rc;
        slot = 0;
    }
    if ((rc = rate_finish(c, job, nf, j, slot, s, h_totals))) return rc;
    for (size_t i = 0; i < seen_j.size(); i++)              // (a quality search's result is a probe the procedure made)
        if (seen_j[i] == j) for (int f = 0; f < nf; f++) h_sse[f] = seen_sse[i * (size_t)nf + (size_t)f];
    *h_j = j;
    return PICSONG_OK;
}

// The entry points' own refusals, over the job they made.  form: which of the three inputs the entry takes; outs: its
// host pointers are all there.  (kOneFrame takes a frame of any alignment, as picsong_encode_frame: an unaligned one
// runs the per-column transform kernels and sse_kernel's per-byte form.)
// kRgbFrames: the n-frame RGB calls -- what picsong_encode_rgb_frames refuses (rgb_frames_refusal), and planes and a
// stride that rgb_sse_kernel's dword loads can take.
enum SearchForm { kFrames, kOneFrame, kRgbFrame, kRgbFrames };

static int search_args_ok(const picsong_ctx *c, const RateJob &job, SearchForm form, SearchKind kind, bool outs, const char *who)
{
    const bool rgb = form == kRgbFrame || form == kRgbFrames;
    REFUSE_DEEP(c, who);
    if (!c || !job.d_streams || !outs || (rgb ? !job.r || !job.g || !job.b : !job.frames)) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    if (form == kRgbFrames) {
        if (const char *why = rgb_frames_refusal(c->p.is_rgb != 0, c->p.cp, true, job.n, job.r, job.g, job.b, job.d_streams, job.frame_stride,
                                                 job.stream_stride, c->P, picsong_max_stream_shorts(c->aw, c->ah)))
            return fail(PICSONG_ERR_ARG, "%s: %s", who, why);
        if ((((uintptr_t)job.r) | ((uintptr_t)job.g) | ((uintptr_t)job.b)) & 3u) return fail(PICSONG_ERR_ARG, "%s: the planes need 4-byte alignment", who);
        if (job.n > 1 && (job.frame_stride & 3u)) return fail(PICSONG_ERR_ARG, "%s: frame_stride must be a multiple of 4", who);
        return PICSONG_OK;
    }
    if (job.n < 1 || job.n > 16) return fail(PICSONG_ERR_ARG, "%s: %d frames outside 1..16", who, job.n);
    const size_t max_shorts = picsong_max_stream_shorts(c->aw, c->ah);
    if (rgb) {
        if (!c->p.is_rgb) return fail(PICSONG_ERR_ARG, "%s: the context is not an RGB one", who);
        if (job.stream_stride < max_shorts) return fail(PICSONG_ERR_ARG, "%s: stream stride smaller than a worst-case codestream", who);
        if ((((uintptr_t)job.r) | ((uintptr_t)job.g) | ((uintptr_t)job.b)) & 3u) return fail(PICSONG_ERR_ARG, "%s: the planes need 4-byte alignment", who);
        return PICSONG_OK;
    }
    if (c->p.is_rgb)
        return fail(PICSONG_ERR_ARG, "%s: grey contexts only (an RGB frame: picsong_encode_rgb_%s)", who,
                    kind == kSearchSize ? "frame_rate" : (kind == kSearchSsim ? "frames_ssim" : "frame_quality"));
    if (job.n > 1 && (job.frame_stride < c->P || job.stream_stride < max_shorts))
        return fail(PICSONG_ERR_ARG, "%s: strides smaller than a padded frame / a worst-case codestream", who);
    if (form == kFrames && (((uintptr_t)job.frames | job.frame_stride) & 15u)) return fail(PICSONG_ERR_ARG, "%s: frames must be 16-byte aligned", who);
    return PICSONG_OK;
}

int picsong_encode_frames_rate(picsong_ctx *c, int n, const uint8_t *d_frames, size_t frame_stride, int first_iter,
                               size_t target_shorts, int j_min, int j_max, uint16_t *d_streams, size_t stream_stride,
                               void *stream, int *h_j, int *h_totals)
{
    const char *who = "encode_frames_rate";
    const RateJob job = { n, d_frames, frame_stride, nullptr, nullptr, nullptr, first_iter, 0, d_streams, stream_stride, false };
    if (int rc = search_args_ok(c, job, kFrames, kSearchSize, h_j && h_totals, who)) return rc;
    return search_impl(c, job, kSearchSize, target_shorts, j_min, j_max, (hipStream_t)stream, h_j, h_totals, nullptr, who);
}

int picsong_encode_frame_rate(picsong_ctx *c, const uint8_t *d_frame, int iter, size_t target_shorts, int j_min, int j_max,
                              uint16_t *d_stream, void *stream, int *h_j, int *h_total)
{
    const char *who = "encode_frame_rate";
    const RateJob job = { 1, d_frame, 0, nullptr, nullptr, nullptr, iter == 0 ? 0 : 1, 0, d_stream, 0, true };
    if (int rc = search_args_ok(c, job, kOneFrame, kSearchSize, h_j && h_total, who)) return rc;
    return search_impl(c, job, kSearchSize, target_shorts, j_min, j_max, (hipStream_t)stream, h_j, h_total, nullptr, who);
}

int picsong_encode_rgb_frame_rate(picsong_ctx *c, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b, int header_mask,
                                  size_t target_shorts, int j_min, int j_max, uint16_t *d_streams, size_t stream_stride,
                                  void *stream, int *h_j, int *h_totals)
{
    const char *who = "encode_rgb_frame_rate";
    const RateJob job = { 1, nullptr, 0, d_r, d_g, d_b, 0, header_mask, d_streams, stream_stride, false };
    if (int rc = search_args_ok(c, job, kRgbFrame, kSearchSize, h_j && h_totals, who)) return rc;
    return search_impl(c, job, kSearchSize, target_shorts, j_min, j_max, (hipStream_t)stream, h_j, h_totals, nullptr, who);
}

int picsong_encode_frames_quality(picsong_ctx *c, int n, const uint8_t *d_frames, size_t frame_stride, int first_iter,
                                  uint64_t max_sse, int j_min, int j_max, uint16_t *d_streams, size_t stream_stride,
                                  void *stream, int *h_j, int *h_totals, uint64_t *h_sse)
{
    const char *who = "encode_frames_quality";
    const RateJob job = { n, d_frames, frame_stride, nullptr, nullptr, nullptr, first_iter, 0, d_streams, stream_stride, false };
    if (int rc = search_args_ok(c, job, kFrames, kSearchQuality, h_j && h_totals && h_sse, who)) return rc;
    return search_impl(c, job, kSearchQuality, max_sse, j_min, j_max, (hipStream_t)stream, h_j, h_totals, h_sse, who);
}

int picsong_encode_frame_quality(picsong_ctx *c, const uint8_t *d_frame, int iter, uint64_t max_sse, int j_min, int j_max,
                                 uint16_t *d_stream, void *stream, int *h_j, int *h_total, uint64_t *h_sse)
{
    const char *who = "encode_frame_quality";
    const RateJob job = { 1, d_frame, 0, nullptr, nullptr, nullptr, iter == 0 ? 0 : 1, 0, d_stream, 0, true };
    if (int rc = search_args_ok(c, job, kOneFrame, kSearchQuality, h_j && h_total && h_sse, who)) return rc;
    return search_impl(c, job, kSearchQuality, max_sse, j_min, j_max, (hipStream_t)stream, h_j, h_total, h_sse, who);
}

int picsong_encode_rgb_frame_quality(picsong_ctx *c, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b, int header_mask,
                                     uint64_t max_sse, int j_min, int j_max, uint16_t *d_streams, size_t stream_stride,
                                     void *stream, int *h_j, int *h_totals, uint64_t *h_sse)
{
    const char *who = "encode_rgb_frame_quality";
    const RateJob job = { 1, nullptr, 0, d_r, d_g, d_b, 0, header_mask, d_streams, stream_stride, false };
    if (int rc = search_args_ok(c, job, kRgbFrame, kSearchQuality, h_j && h_totals && h_sse, who)) return rc;
    return search_impl(c, job, kSearchQuality, max_sse, j_min, j_max, (hipStream_t)stream, h_j, h_totals, h_sse, who);
}

// The n-frame RGB calls: frame f's planes frame_stride bytes after d_r / d_g / d_b, its component k's stream at
// (3 f + k) * stream_stride; size(j) and sse(j) the sums over the 3 n planes.
int picsong_encode_rgb_frames_rate(picsong_ctx *c, int n, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b, size_t frame_stride,
                                   int first_iter, int header_mask, size_t target_shorts, int j_min, int j_max, uint16_t *d_streams,
                                   size_t stream_stride, void *stream, int *h_j, int *h_totals)
{
    const char *who = "encode_rgb_frames_rate";
    RateJob job = { n, nullptr, n > 1 ? frame_stride : 0, d_r, d_g, d_b, first_iter, header_mask, d_streams, stream_stride, false };
    job.multi = true;
    if (int rc = search_args_ok(c, job, kRgbFrames, kSearchSize, h_j && h_totals, who)) return rc;
    return search_impl(c, job, kSearchSize, target_shorts, j_min, j_max, (hipStream_t)stream, h_j, h_totals, nullptr, who);
}

int picsong_encode_rgb_frames_quality(picsong_ctx *c, int n, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b, size_t frame_stride,
                                      int first_iter, int header_mask, uint64_t max_sse, int j_min, int j_max, uint16_t *d_streams,
                                      size_t stream_stride, void *stream, int *h_j, int *h_totals, uint64_t *h_sse)
{
    const char *who = "encode_rgb_frames_quality";
    RateJob job = { n, nullptr, n > 1 ? frame_stride : 0, d_r, d_g, d_b, first_iter, header_mask, d_streams, stream_stride, false };
    job.multi = true;
    if (int rc = search_args_ok(c, job, kRgbFrames, kSearchQuality, h_j && h_totals && h_sse, who)) return rc;
    return search_impl(c, job, kSearchQuality, max_sse, j_min, j_max, (hipStream_t)stream, h_j, h_totals, h_sse, who);
}

// ---- the SSIM calls: the quality calls with the DSSIM sum (ssim_kernel, quality_kernels.hpp) for the SSE.  The probe
// is quality_probe's with frames_dssim as its last step; an RGB probe takes the unfused tail (rgb_inverse into q_pix).
int picsong_ssim_windows(int w, int h, uint64_t *windows)
{
    if (!windows) return fail(PICSONG_ERR_ARG, "ssim_windows: null argument");
    if (!ssim_geometry_ok(w, h)) return fail(PICSONG_ERR_ARG, "ssim_windows: %d x %d is below the 8 x 8 of a window", w, h);
    *windows = ssim_windows(w, h);
    return PICSONG_OK;
}

int picsong_ssim_to_dssim(double ssim, uint64_t windows, uint64_t *max_dssim)
{
    if (!max_dssim) return fail(PICSONG_ERR_ARG, "ssim_to_dssim: null argument");
    if (windows == 0) return fail(PICSONG_ERR_ARG, "ssim_to_dssim: no windows");
    if (!(ssim >= -1.0 && ssim <= 1.0)) return fail(PICSONG_ERR_ARG, "ssim_to_dssim: the SSIM must lie in [-1, 1]");
    const double v = std::floor(((1.0 - ssim) * (double)windows) * 16777216.0);
    *max_dssim = v >= 18446744073709551615.0 ? UINT64_MAX : (uint64_t)v;
    return PICSONG_OK;
}

int picsong_dssim_to_ssim(uint64_t dssim, uint64_t windows, double *ssim)
{
    if (!ssim) return fail(PICSONG_ERR_ARG, "dssim_to_ssim: null argument");
    if (windows == 0) return fail(PICSONG_ERR_ARG, "dssim_to_ssim: no windows");
    *ssim = 1.0 - (double)dssim / ((double)windows * 16777216.0);
    return PICSONG_OK;
}

int picsong_frames_dssim(picsong_ctx *c, int n, const uint8_t *d_a, size_t a_stride, const uint8_t *d_b, size_t b_stride,
                         uint64_t *d_dssim, void *stream)
{
    REFUSE_DEEP(c, "frames_dssim");
    if (!c || !d_a || !d_b || !d_dssim) return fail(PICSONG_ERR_ARG, "frames_dssim: null argument");
    if (n < 1 || n > kSseMaxFrames) return fail(PICSONG_ERR_ARG, "frames_dssim: %d frames outside 1..%d", n, kSseMaxFrames);
    if (n > 1 && (a_stride < c->P || b_stride < c->P)) return fail(PICSONG_ERR_ARG, "frames_dssim: strides smaller than a padded frame");
    if (!ssim_geometry_ok(c->p.width, c->p.height)) return fail(PICSONG_ERR_ARG, "frames_dssim: the SSIM's 8 x 8 windows need a frame of 8 x 8 or more");
    HIP_TRY(hipSetDevice(c->device));
    return frames_dssim(HipGo{ (hipStream_t)stream }, d_a, (size_t)c->aw, n > 1 ? a_stride : 0, d_b, (size_t)c->aw, n > 1 ? b_stride : 0,
                        c->p.width, c->p.height, n, reinterpret_cast<unsigned long long *>(d_dssim));
}

int picsong_encode_frames_ssim(picsong_ctx *c, int n, const uint8_t *d_frames, size_t frame_stride, int first_iter,
                               uint64_t max_dssim, int j_min, int j_max, uint16_t *d_streams, size_t stream_stride,
                               void *stream, int *h_j, int *h_totals, uint64_t *h_dssim)
{
    const char *who = "encode_frames_ssim";
    const RateJob job = { n, d_frames, frame_stride, nullptr, nullptr, nullptr, first_iter, 0, d_streams, stream_stride, false };
    if (int rc = search_args_ok(c, job, kFrames, kSearchSsim, h_j && h_totals && h_dssim, who)) return rc;
    return search_impl(c, job, kSearchSsim, max_dssim, j_min, j_max, (hipStream_t)stream, h_j, h_totals, h_dssim, who);
}

int picsong_encode_frame_ssim(picsong_ctx *c, const uint8_t *d_frame, int iter, uint64_t max_dssim, int j_min, int j_max,
                              uint16_t *d_stream, void *stream, int *h_j, int *h_total, uint64_t *h_dssim)
{
    const char *who = "encode_frame_ssim";
    const RateJob job = { 1, d_frame, 0, nullptr, nullptr, nullptr, iter == 0 ? 0 : 1, 0, d_stream, 0, true };
    if (int rc = search_args_ok(c, job, kOneFrame, kSearchSsim, h_j && h_total && h_dssim, who)) return rc;
    return search_impl(c, job, kSearchSsim, max_dssim, j_min, j_max, (hipStream_t)stream, h_j, h_total, h_dssim, who);
}

int picsong_encode_rgb_frames_ssim(picsong_ctx *c, int n, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b, size_t frame_stride,
                                   int first_iter, int header_mask, uint64_t max_dssim, int j_min, int j_max, uint16_t *d_streams,
                                   size_t stream_stride, void *stream, int *h_j, int *h_totals, uint64_t *h_dssim)
{
    const char *who = "encode_rgb_frames_ssim";
    RateJob job = { n, nullptr, n > 1 ? frame_stride : 0, d_r, d_g, d_b, first_iter, header_mask, d_streams, stream_stride, false };
    job.multi = true;
    if (int rc = search_args_ok(c, job, kRgbFrames, kSearchSsim, h_j && h_totals && h_dssim, who)) return rc;
    return search_impl(c, job, kSearchSsim, max_dssim, j_min, j_max, (hipStream_t)stream, h_j, h_totals, h_dssim, who);
}

// ---------------------------------------------------------------------------------------------
// training: the statistics of the two-pass coder's decisions (train_kernels.hpp) and the tables made from them
// ---------------------------------------------------------------------------------------------
static int train_ready(const picsong_ctx *c, const char *who)
{
    if (!c) return fail(PICSONG_ERR_ARG, "%s: null context", who);
    if (!c->train_on) return fail(PICSONG_ERR_ARG, "%s: call picsong_train_begin first", who);
    return PICSONG_OK;
}

static void train_free(picsong_ctx *c)
{
    for (int k = 0; k < 3; k++) {
        if (c->d_train[k]) (void)hipFree(c->d_train[k]);
        c->d_train[k] = nullptr;
    }
    c->train_on = false;
    c->train_total = 0;
}

int picsong_train_begin(picsong_ctx *c, const picsong_lut_info *geo)
{
    if (!c || !geo) return fail(PICSONG_ERR_ARG, "train_begin: null argument");
    if (c->p.cp == 3) return fail(PICSONG_ERR_ARG, "train_begin: -cp 3 contexts code other decisions (cp_sig / cp_sign): not trained");
    if (c->p.k > 0.0f) return fail(PICSONG_ERR_ARG, "train_begin: -k > 0 contexts code from the bit-plane files _1.._14: not trained");
    if (geo->n_bitplanes < 1 || geo->n_subbands < 1 || geo->ctx_ref < 1 || geo->ctx_sig < 1 || geo->ctx_sign < 1)
        return fail(PICSONG_ERR_ARG, "train_begin: geometry %d bit-planes, %d subbands, %d/%d/%d contexts (ref/sig/sign): each must be >= 1",
                    geo->n_bitplanes, geo->n_subbands, geo->ctx_ref, geo->ctx_sig, geo->ctx_sign);
    if (geo->n_ref < 0 || geo->n_sig < 0 || geo->n_sign < 0) return fail(PICSONG_ERR_ARG, "train_begin: negative section size");
    picsong_lut_info li = *geo;
    // section sizes of 0 follow from the geometry and the context's wl (64-bit: a geometry of large numbers must not
    // wrap on its way to the refusal)
    const long long planes = ((long long)li.n_subbands * c->p.wl + 1) * li.n_bitplanes;
    const long long n_ref = li.n_ref > 0 ? li.n_ref : planes * li.ctx_ref, n_sig = li.n_sig > 0 ? li.n_sig : planes * li.ctx_sig,
                    n_sign = li.n_sign > 0 ? li.n_sign : planes * li.ctx_sign;
    const long long total = n_ref + n_sig + n_sign;
    if (planes > kTrainMaxEntries || total > kTrainMaxEntries)
        return fail(PICSONG_ERR_ARG, "train_begin: a table of %lld entries exceeds the %d a workgroup's copy holds", total, kTrainMaxEntries);
    LutGeo g = lut_geo(li);
    g.nRef = (int)n_ref; g.nSig = (int)n_sig; g.nSign = (int)n_sign;
    li.n_ref = g.nRef; li.n_sig = g.nSig; li.n_sign = g.nSign;
    li.n_files = 3; li.n_bp_files = 1; li.n_tables = 1; li.cp = 2;
    HIP_TRY(hipSetDevice(c->device));
    if (c->train_on) { HIP_TRY(hipDeviceSynchronize()); train_free(c); }
    const size_t bytes = (size_t)total * 2 * sizeof(unsigned long long);
    for (int k = 0; k < 3; k++) {
        hipError_t e = hipMalloc(&c->d_train[k], bytes);
        if (e == hipSuccess) e = hipMemset(c->d_train[k], 0, bytes);
        if (e != hipSuccess) { train_free(c); return fail(PICSONG_ERR_HIP, "train_begin: %s", hipGetErrorString(e)); }
    }
    c->train_li = li;
    c->train_total = (int)total;
    c->train_on = true;
    return PICSONG_OK;
}

int picsong_train_info(const picsong_ctx *c, picsong_lut_info *info)
{
    if (int rc = train_ready(c, "train_info")) return rc;
    if (!info) return fail(PICSONG_ERR_ARG, "train_info: null argument");
    *info = c->train_li;
    return PICSONG_OK;
}

int picsong_train_reset(picsong_ctx *c)
{
    if (int rc = train_ready(c, "train_reset")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());                        // (no stream argument: calls in flight on any stream count first)
    for (int k = 0; k < 3; k++) HIP_TRY(hipMemset(c->d_train[k], 0, (size_t)c->train_total * 2 * sizeof(unsigned long long)));
    return PICSONG_OK;
}

int picsong_train_end(picsong_ctx *c)
{
    if (int rc = train_ready(c, "train_end")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    train_free(c);
    if (c->train_scratch) (void)hipFree(c->train_scratch);
    c->train_scratch = nullptr; c->train_scratch_dwords = 0;
    return PICSONG_OK;
}

// The statistics launch of every path: `frames` coefficient arrays coef_z bytes apart into slot comp's counters
static int launch_stats(picsong_ctx *c, int comp, const void *d_coeffs, bool c16, int frames, unsigned long long coef_z, hipStream_t s)
{
    const size_t pairs = (size_t)frames * (size_t)((c->ncb + 1) / 2);
    const StatsLaunch l = select_stats(pairs);
    if (!train_pairs_ok(pairs, l.wgs)) return fail(PICSONG_ERR_ARG, "train: %zu codeblock pairs in one launch", pairs);
    if (c->train_scratch_dwords < l.scratch_dwords) {
        HIP_TRY(hipDeviceSynchronize());                    // a smaller launch may still be running on the old scratch
        if (c->train_scratch) (void)hipFree(c->train_scratch);
        c->train_scratch = nullptr; c->train_scratch_dwords = 0;
        HIP_TRY(hipMalloc(&c->train_scratch, l.scratch_dwords * sizeof(uint32_t)));
        c->train_scratch_dwords = l.scratch_dwords;
    }
    const BpcArgs a = stats_args(c->aw, c->ah, c->p.wl, lut_geo(c->train_li), c->d_flag, d_coeffs, c->p.lossy != 0 && !c16, c16,
                                 frames, coef_z, c->train_scratch);
    return HipGo{ s }(l.kernel, dim3(l.wgs), l.threads, a, c->d_train[comp], (int)pairs);
}

int picsong_train_coeffs(picsong_ctx *c, int comp, const void *d_coeffs, void *stream)
{
    if (int rc = train_ready(c, "train_coeffs")) return rc;
    if (!d_coeffs) return fail(PICSONG_ERR_ARG, "train_coeffs: null argument");
    if (comp < 0 || comp > 2) return fail(PICSONG_ERR_ARG, "train_coeffs: component %d outside 0..2", comp);
    HIP_TRY(hipSetDevice(c->device));
    return launch_stats(c, comp, d_coeffs, false, 1, 0, (hipStream_t)stream);
}

int picsong_train_frames(picsong_ctx *c, int n, const uint8_t *d_frames, size_t frame_stride, void *stream)
{
    REFUSE_DEEP(c, "train_frames");
    if (int rc = train_ready(c, "train_frames")) return rc;
    if (!d_frames) return fail(PICSONG_ERR_ARG, "train_frames: null argument");
    if (n < 1 || n > 64) return fail(PICSONG_ERR_ARG, "train_frames: %d frames outside 1..64", n);
    if (n > 1 && frame_stride < c->P) return fail(PICSONG_ERR_ARG, "train_frames: stride smaller than a padded frame");
    if (c->p.is_rgb) return fail(PICSONG_ERR_ARG, "train_frames: grey contexts only (an RGB frame's components: picsong_train_rgb_frame)");
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_batch(c, n);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t coef_z = (c->P + c->extra) * 4;
    bool c16 = false;
    if (((((uintptr_t)d_frames) | frame_stride) & 15u) == 0) {
        // ---- the transform of picsong_encode_frames: frame 0's plan with grid.z = n
        std::vector<FwdLaunch> plan = plan_dwt_forward(d_frames, true, c->batch.coef, c->aw, c->ah, c->p.wl, c->p.qs, c->c16);
        c16 = plan_is_c16(plan);
        plan_frame_strides(plan, frame_stride, coef_z);
        if ((rc = launch_fwd_plan(HipGo{ s }, c->p.lossy != 0, plan, (unsigned)n))) return rc;
    } else {
        // ---- frames whose alignment differs from one another: a plan each, the 32-bit arrays for all of them
        for (int f = 0; f < n; f++) {
            const std::vector<FwdLaunch> plan = plan_dwt_forward(d_frames + (size_t)f * frame_stride, true, (char *)c->batch.coef + (size_t)f * coef_z,
                                                                 c->aw, c->ah, c->p.wl, c->p.qs, false);
            if ((rc = launch_fwd_plan(HipGo{ s }, c->p.lossy != 0, plan))) return rc;
        }
    }
    return launch_stats(c, 0, c->batch.coef, c16, n, coef_z, s);
}

int picsong_train_rgb_frame(picsong_ctx *c, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b, void *stream)
{
    REFUSE_DEEP(c, "train_rgb_frame");
    if (int rc = train_ready(c, "train_rgb_frame")) return rc;
    if (!d_r || !d_g || !d_b) return fail(PICSONG_ERR_ARG, "train_rgb_frame: null argument");
    if (!c->p.is_rgb) return fail(PICSONG_ERR_ARG, "train_rgb_frame: the context is not an RGB one");
    if ((((uintptr_t)d_r) | ((uintptr_t)d_g) | ((uintptr_t)d_b)) & 3u) return fail(PICSONG_ERR_ARG, "train_rgb_frame: the planes need 4-byte alignment");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_batch(c, 3))) return rc;
    if ((rc = ensure_coef_i(c, 3))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t coef_z = (c->P + c->extra) * 4;
    bool c16 = false;
    if ((rc = rgb_forward_transform(c, d_r, d_g, d_b, s, &c16))) return rc;
    // (a launch a component: a workgroup's on-chip copy of the counters belongs to one slot)
    for (int k = 0; k < 3; k++)
        if ((rc = launch_stats(c, k, (const char *)c->batch.coef + (size_t)k * coef_z, c16, 1, 0, s))) return rc;
    return PICSONG_OK;
}

// n RGB frames: one transform of the 3 n planes, then a statistics launch a component over its n arrays (component k's
// start at plane k, 3 planes apart).  The counts are those of n picsong_train_rgb_frame calls.
int picsong_train_rgb_frames(picsong_ctx *c, int n, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b, size_t frame_stride,
                             void *stream)
{
    REFUSE_DEEP(c, "train_rgb_frames");
    if (int rc = train_ready(c, "train_rgb_frames")) return rc;
    if (!d_r || !d_g || !d_b) return fail(PICSONG_ERR_ARG, "train_rgb_frames: null argument");
    if (!c->p.is_rgb) return fail(PICSONG_ERR_ARG, "train_rgb_frames: the context is not an RGB one");
    if ((((uintptr_t)d_r) | ((uintptr_t)d_g) | ((uintptr_t)d_b)) & 3u) return fail(PICSONG_ERR_ARG, "train_rgb_frames: the planes need 4-byte alignment");
    if (n < 1 || n > kRgbMaxFrames) return fail(PICSONG_ERR_ARG, "train_rgb_frames: %d frames outside 1..%d", n, kRgbMaxFrames);
    if (n > 1 && (frame_stride < c->P || (frame_stride & 3u)))
        return fail(PICSONG_ERR_ARG, "train_rgb_frames: frame_stride smaller than a padded plane, or no multiple of 4");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_batch(c, 3 * n))) return rc;
    if ((rc = ensure_coef_i(c, 3 * n))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t coef_z = (c->P + c->extra) * 4;
    bool c16 = false;
    if ((rc = rgb_forward_transform(c, d_r, d_g, d_b, s, &c16, n, n > 1 ? frame_stride : 0))) return rc;
    for (int k = 0; k < 3; k++)
        if ((rc = launch_stats(c, k, (const char *)c->batch.coef + (size_t)k * coef_z, c16, n, 3ull * coef_z, s))) return rc;
    return PICSONG_OK;
}

int picsong_train_counts(picsong_ctx *c, int comp, void *stream, uint64_t *h_counts, size_t capacity_entries)
{
    if (int rc = train_ready(c, "train_counts")) return rc;
    if (comp < 0 || comp > 2) return fail(PICSONG_ERR_ARG, "train_counts: component %d outside 0..2", comp);
    if (!h_counts) return c->train_total;
    if (capacity_entries < (size_t)c->train_total)
        return fail(PICSONG_ERR_ARG, "train_counts: capacity %zu < %d entries", capacity_entries, c->train_total);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(h_counts, c->d_train[comp], (size_t)c->train_total * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PICSONG_OK;
}

// ---- host only: counts -> table -> folder
static int lut_info_complete(const picsong_lut_info *info, const char *who)
{
    if (info->n_bitplanes < 1 || info->n_subbands < 1 || info->ctx_ref < 1 || info->ctx_sig < 1 || info->ctx_sign < 1)
        return fail(PICSONG_ERR_ARG, "%s: geometry fields must be >= 1", who);
    if (info->ctx_ref > 16 || info->ctx_sig > 16 || info->ctx_sign > 16) return fail(PICSONG_ERR_ARG, "%s: context counts above 16 are not supported", who);
    if (info->precision < 1 || info->precision > 8) return fail(PICSONG_ERR_ARG, "%s: precision %d outside 1..8", who, info->precision);
    if (info->n_ref < 1 || info->n_sig < 1 || info->n_sign < 1)
        return fail(PICSONG_ERR_ARG, "%s: section sizes missing (picsong_train_info / picsong_lut_load fill them in)", who);
    return PICSONG_OK;
}

int picsong_lut_from_counts(const picsong_lut_info *info, const uint64_t *counts, const int32_t *prior, int32_t *table)
{
    if (!info || !counts || !table) return fail(PICSONG_ERR_ARG, "lut_from_counts: null argument");
    if (int rc = lut_info_complete(info, "lut_from_counts")) return rc;
    const size_t total = (size_t)info->n_ref + info->n_sig + info->n_sign;
    const int prec = info->precision;
    const uint64_t top = ((uint64_t)1 << prec) - 1;
    for (size_t i = 0; i < total; i++) {
        const uint64_t z = counts[2 * i], o = counts[2 * i + 1], t = z + o;
        if (t == 0) { table[i] = prior ? prior[i] : (int32_t)(1 << (prec - 1)); continue; }
        if (t < z || z > (~(uint64_t)0 >> (prec + 1))) return fail(PICSONG_ERR_ARG, "lut_from_counts: entry %zu's counts overflow 64 bits", i);
        uint64_t p = ((z << prec) + t / 2) / t;
        p = p < 1 ? 1 : (p > top ? top : p);
        table[i] = (int32_t)p;
    }
    return PICSONG_OK;
}

int picsong_lut_save(const char *folder_c, int component, const picsong_lut_info *info, int wl, const int32_t *table)
{
    if (!folder_c || !info || !table || !*folder_c) return fail(PICSONG_ERR_ARG, "lut_save: null argument");
    if (component < 0 || component > 3) return fail(PICSONG_ERR_ARG, "lut_save: component %d outside 0..3", component);
    if (wl < 1 || wl > 10) return fail(PICSONG_ERR_ARG, "lut_save: wl %d out of range", wl);
    if (int rc = lut_info_complete(info, "lut_save")) return rc;
    const int nB = info->n_bitplanes, nS = info->n_subbands, groups = nS * wl + 1;
    if (info->n_ref != groups * nB * info->ctx_ref || info->n_sig != groups * nB * info->ctx_sig || info->n_sign != groups * nB * info->ctx_sign)
        return fail(PICSONG_ERR_ARG, "lut_save: the section sizes %d/%d/%d are not those of wl %d (%d groups of %d planes)", info->n_ref,
                    info->n_sig, info->n_sign, wl, groups, nB);
    std::string folder(folder_c);
    if (folder.back() != '/') folder += '/';
    if (mkdir(folder.c_str(), 0777) != 0 && errno != EEXIST) return fail(PICSONG_ERR_IO, "lut_save: cannot create %s: %s", folder.c_str(), strerror(errno));
    FILE *f = fopen((folder + "header.txt").c_str(), "wb");
    if (!f) return fail(PICSONG_ERR_IO, "lut_save: cannot write %sheader.txt: %s", folder.c_str(), strerror(errno));
    fprintf(f, "LUT_N_BITPLANES;%d\nLUT_N_SUBBANDS;%d\nN_CONTEXT_REFINEMENT;%d\nN_CONTEXT_SIGN;%d\nN_CONTEXT_SIGNIFICANCE;%d\n"
               "MULT_PRECISION;%d\nLUT_N_FILES;3\nAMOUNT_OF_BITPLANE_FILES;1\n", nB, nS, info->ctx_ref, info->ctx_sign, info->ctx_sig, info->precision);
    if (fclose(f) != 0) return fail(PICSONG_ERR_IO, "lut_save: writing %sheader.txt failed", folder.c_str());
    static const char *suffix[4] = { ".txt_0", "R.txt_0", "G.txt_0", "B.txt_0" };
    const struct { const char *stem; int C, base; } sec[3] = { { "ref", info->ctx_ref, 0 }, { "sig", info->ctx_sig, info->n_ref },
                                                               { "sign", info->ctx_sign, info->n_ref + info->n_sig } };
    for (int k = 0; k < 3; k++) {
        const std::string path = folder + sec[k].stem + suffix[component];
        if (!(f = fopen(path.c_str(), "wb"))) return fail(PICSONG_ERR_IO, "lut_save: cannot write %s: %s", path.c_str(), strerror(errno));
        const int32_t *T = table + sec[k].base;
        for (int grp = 0; grp < groups; grp++)
            for (int bp = 0; bp < nB; bp++) {
                fprintf(f, "%d %d %d : ", grp / nS, grp % nS, bp);
                for (int x = 0; x < sec[k].C; x++) fprintf(f, "%d ", T[((size_t)grp * nB + bp) * sec[k].C + x]);
                fputc('\n', f);
            }
        if (fclose(f) != 0) return fail(PICSONG_ERR_IO, "lut_save: writing %s failed", path.c_str());
    }
    return PICSONG_OK;
}

// ---------------------------------------------------------------------------------------------
// frames as applications hold them (layout_kernels.hpp): pitched, unpadded, interleaved images to and from the padded
// planar planes, on the device; the whole-frame calls run the plain frame sequences behind / before them
// ---------------------------------------------------------------------------------------------
static int layout_args_ok(const picsong_ctx *c, int n, const picsong_image *img, size_t frame_stride, const void *d_padded,
                          size_t padded_stride, const char *who)
{
    if (!c || !img) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    if (const char *why = layout_refusal(img->layout, img->data, img->pitch, img->plane_stride, frame_stride, d_padded, padded_stride, n,
                                         c->p.width, c->p.height, c->aw, c->ah, is_deep(c), is_deep_rgb(c)))
        return fail(PICSONG_ERR_ARG, "%s: %s", who, why);
    return PICSONG_OK;
}

int picsong_ingest_frames(picsong_ctx *c, int n, const picsong_image *src, size_t frame_stride, uint8_t *d_padded,
                          size_t padded_stride, void *stream)
{
    if (int rc = layout_args_ok(c, n, src, frame_stride, d_padded, padded_stride, "ingest_frames")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return ingest_frames(HipGo{ (hipStream_t)stream }, src->layout, src->data, src->pitch, src->plane_stride, frame_stride, d_padded,
                         padded_stride, n, c->p.width, c->p.height, c->aw, c->ah, nullptr, is_deep(c) ? px_max(c) : 0);
}

int picsong_emit_frames(picsong_ctx *c, int n, const uint8_t *d_padded, size_t padded_stride, const picsong_image *dst,
                        size_t frame_stride, void *stream)
{
    if (int rc = layout_args_ok(c, n, dst, frame_stride, d_padded, padded_stride, "emit_frames")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return emit_frames(HipGo{ (hipStream_t)stream }, dst->layout, d_padded, padded_stride, dst->data, dst->pitch, dst->plane_stride,
                       frame_stride, n, c->p.width, c->p.height, c->aw, c->ah, nullptr, is_deep(c) ? px_max(c) : 0);
}

// the context's padded planes for the image calls: `planes` of P bytes (hipMalloc: 256-byte aligned)
static int ensure_layout(picsong_ctx *c, size_t planes)
{
    if (planes * c->P <= c->lay_cap) return PICSONG_OK;
    HIP_TRY(hipDeviceSynchronize());                 // an earlier call may still be running on the old buffer
    if (c->lay_buf) (void)hipFree(c->lay_buf);
    c->lay_buf = nullptr; c->lay_cap = 0;
    HIP_TRY(hipMalloc(&c->lay_buf, planes * c->P));
    c->lay_cap = planes * c->P;
    return PICSONG_OK;
}
// what the image calls check before anything is launched: the layout arguments (the padded side is the context's own
// buffer) and the layout against the context's colour mode
static int image_args_ok(const picsong_ctx *c, int n, const picsong_image *img, size_t frame_stride, const void *d_streams, bool rgb,
                         const char *who)
{
    if (!c || !img || !d_streams) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    // (the padded side is the context's buffer, allocated later: any non-null address stands for it, its stride a frame's planes)
    if (int rc = layout_args_ok(c, n, img, frame_stride, c, (size_t)(is_deep_rgb(c) ? 6 : 3) * c->P, who)) return rc;
    if (is_deep_rgb(c))                                     // (16-bit colour layouts: the n-frame RGB image calls alone)
        return fail(PICSONG_ERR_ARG, "%s: a %d-bit RGB context's image calls are picsong_encode_rgb_images / picsong_decode_rgb_images",
                    who, c->p.bit_depth);
    if (img->layout == kLayoutGrey16) {                     // (a deep context: layout_args_ok; grey by its creation)
        if (rgb) return fail(PICSONG_ERR_ARG, "%s: the context is not an RGB one", who);
        if (c->p.cp == 3) return fail(PICSONG_ERR_ARG, "%s: -cp 2 contexts only, as the frame call behind it", who);
        return PICSONG_OK;
    }
    if (rgb != (c->p.is_rgb != 0)) return fail(PICSONG_ERR_ARG, "%s: the context is %s", who, rgb ? "not an RGB one" : "an RGB one");
    if (rgb != (img->layout != kLayoutGrey8))
        return fail(PICSONG_ERR_ARG, "%s: layout %d on %s context", who, img->layout, rgb ? "an RGB" : "a grey");
    if (c->p.cp == 3) return fail(PICSONG_ERR_ARG, "%s: -cp 2 contexts only, as the frame call behind it", who);
    return PICSONG_OK;
}

int picsong_encode_images(picsong_ctx *c, int n, const picsong_image *src, size_t frame_stride, int first_iter, uint16_t *d_streams,
                          size_t stream_stride, void *stream)
{
    const char *who = "encode_images";
    if (int rc = image_args_ok(c, n, src, frame_stride, d_streams, false, who)) return rc;
    if (n > 1 && stream_stride < picsong_max_stream_shorts(c->aw, c->ah))
        return fail(PICSONG_ERR_ARG, "%s: stream stride smaller than a worst-case codestream", who);
    BpcArgs a;
    if (int rc = bpc_args(c, a, 0)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bps = is_deep(c) ? 2 : 1;                  // bytes a padded sample
    if (int rc = ensure_layout(c, (size_t)n * bps)) return rc;
    if (int rc = ingest_frames(HipGo{ (hipStream_t)stream }, src->layout, src->data, src->pitch, src->plane_stride, frame_stride, c->lay_buf,
                               bps * c->P, n, c->p.width, c->p.height, c->aw, c->ah)) return rc;
    if (is_deep(c))
        return picsong_encode_frames16(c, n, reinterpret_cast<const uint16_t *>(c->lay_buf), 2 * c->P, first_iter, d_streams, stream_stride, stream);
    return picsong_encode_frames(c, n, c->lay_buf, c->P, first_iter, d_streams, stream_stride, stream);
}

int picsong_decode_images(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, const picsong_image *dst,
                          size_t frame_stride, void *stream)
{
    const char *who = "decode_images";
    if (int rc = image_args_ok(c, n, dst, frame_stride, d_streams, false, who)) return rc;
    if (n > 1 && stream_stride < picsong_max_stream_shorts(c->aw, c->ah))
        return fail(PICSONG_ERR_ARG, "%s: stream stride smaller than a worst-case codestream", who);
    BpcArgs a;
    if (int rc = bpc_args(c, a, 0)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bps = is_deep(c) ? 2 : 1;
    if (int rc = ensure_layout(c, (size_t)n * bps)) return rc;
    if (is_deep(c)) {
        if (int rc = picsong_decode_frames16(c, n, d_streams, stream_stride, reinterpret_cast<uint16_t *>(c->lay_buf), 2 * c->P, stream)) return rc;
    } else if (int rc = picsong_decode_frames(c, n, d_streams, stream_stride, c->lay_buf, c->P, stream)) return rc;
    return emit_frames(HipGo{ (hipStream_t)stream }, dst->layout, c->lay_buf, bps * c->P, dst->data, dst->pitch, dst->plane_stride, frame_stride,
                       n, c->p.width, c->p.height, c->aw, c->ah);
}

int picsong_encode_rgb_image(picsong_ctx *c, const picsong_image *src, int header_mask, uint16_t *d_streams, size_t stream_stride,
                             void *stream)
{
    const char *who = "encode_rgb_image";
    REFUSE_DEEP(c, who);
    if (int rc = image_args_ok(c, 1, src, 0, d_streams, true, who)) return rc;
    if (stream_stride < picsong_max_stream_shorts(c->aw, c->ah))
        return fail(PICSONG_ERR_ARG, "%s: stream stride smaller than a worst-case codestream", who);
    BpcArgs a;
    if (int rc = bpc_args_rgb(c, a)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_layout(c, 3)) return rc;
    if (int rc = ingest_frames(HipGo{ (hipStream_t)stream }, src->layout, src->data, src->pitch, src->plane_stride, 0, c->lay_buf, 0, 1,
                               c->p.width, c->p.height, c->aw, c->ah)) return rc;
    return picsong_encode_rgb_frame(c, c->lay_buf, c->lay_buf + c->P, c->lay_buf + 2 * c->P, header_mask, d_streams, stream_stride, stream);
}

int picsong_decode_rgb_image(picsong_ctx *c, const uint16_t *d_streams, size_t stream_stride, const picsong_image *dst, void *stream)
{
    const char *who = "decode_rgb_image";
    REFUSE_DEEP(c, who);
    if (int rc = image_args_ok(c, 1, dst, 0, d_streams, true, who)) return rc;
    if (stream_stride < picsong_max_stream_shorts(c->aw, c->ah))
        return fail(PICSONG_ERR_ARG, "%s: stream stride smaller than a worst-case codestream", who);
    BpcArgs a;
    if (int rc = bpc_args_rgb(c, a)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_layout(c, 3)) return rc;
    if (int rc = picsong_decode_rgb_frame(c, d_streams, stream_stride, c->lay_buf, c->lay_buf + c->P, c->lay_buf + 2 * c->P, stream)) return rc;
    return emit_frames(HipGo{ (hipStream_t)stream }, dst->layout, c->lay_buf, 0, dst->data, dst->pitch, dst->plane_stride, 0, 1,
                       c->p.width, c->p.height, c->aw, c->ah);
}

// ---------------------------------------------------------------------------------------------
// batched RGB frames: n colour frames through ONE launch per stage, 3 n planes a launch -- plane z = component z % 3 of
// frame z / 3 (the sequences: rgb_forward_transform and decode_rgb_frames, launch_seq.hpp; the argument checks:
// rgb_frames_refusal and its proxy forms, kernel_select.hpp).  The single-frame calls (picsong_encode_rgb_frame,
// picsong_decode_rgb_frame and its _reduced and _window forms) are the n = 1 case: frame_stride 0, first_iter 0.
// ---------------------------------------------------------------------------------------------
static int rgb_frames_args(picsong_ctx *c, int n, const void *r, const void *g, const void *b, const void *streams, size_t frame_stride,
                           size_t stream_stride, const char *who, BpcArgs &a)
{
    if (!c) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    if (const char *why = rgb_frames_refusal(c->p.is_rgb != 0, c->p.cp, true, n, r, g, b, streams, frame_stride, stream_stride, c->P,
                                             picsong_max_stream_shorts(c->aw, c->ah)))
        return fail(PICSONG_ERR_ARG, "%s: %s", who, why);
    if (int rc = bpc_args_rgb(c, a)) return rc;             // (the tables' geometry)
    a.frames = 3 * n;
    return PICSONG_OK;
}

// The tail of the n-frame colour encode calls, 8-bit and deep alike, behind the transform of the 3 n planes into batch.coef
// (c16: as int16 Mallat arrays): the coder, one grid over the planes' codeblock pairs, plane z with table z % 3; then the
// pack, the populated header on the components of header_mask, on the video's frame 0 where the call holds it
static int rgb_code_and_pack(picsong_ctx *c, BpcArgs &a, int n, bool c16, int first_iter, int header_mask, uint16_t *d_streams,
                             size_t stream_stride, hipStream_t s)
{
    const unsigned np = 3u * (unsigned)n;
    a.c16 = c16 ? 1 : 0;
    a.coeffs_in = c->batch.coef; a.is_float = c->p.lossy ? 1 : 0;
    a.staging16 = reinterpret_cast<uint16_t *>(c->batch.staging);
    a.sizes = c->batch.sizes; a.plane_scratch = c->batch.plane_scratch; a.coef_z = (c->P + c->extra) * 4;
    if (int rc = launch_encoder(c, a, np * (unsigned)a.waves_per_frame, 0, 3, s)) return rc;
    uint16_t hdr[PICSONG_HDR_SHORTS];
    picsong_header_pack(&c->p, hdr);
    if (int rc = pack_rgb_frames(HipGo{ s }, a.staging16, c->batch, c->ncb, (unsigned)n, hdr, first_iter, header_mask, d_streams, c->P,
                                 stream_stride)) return rc;
    c->last_batch = (int)np;
    return PICSONG_OK;
}

static int encode_rgb_frames_impl(picsong_ctx *c, int n, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b, size_t frame_stride,
                                  int first_iter, int header_mask, uint16_t *d_streams, size_t stream_stride, void *stream, const char *who)
{
    REFUSE_DEEP(c, who);
    BpcArgs a;
    int rc = rgb_frames_args(c, n, d_r, d_g, d_b, d_streams, frame_stride, stream_stride, who, a);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const unsigned np = 3u * (unsigned)n;
    if ((rc = ensure_batch(c, (int)np))) return rc;
    if ((rc = ensure_coef_i(c, (int)np))) return rc;
    hipStream_t s = (hipStream_t)stream;
    bool c16 = false;
    if ((rc = rgb_forward_transform(c, d_r, d_g, d_b, s, &c16, n, frame_stride))) return rc;
    return rgb_code_and_pack(c, a, n, c16, first_iter, header_mask, d_streams, stream_stride, s);
}

int picsong_encode_rgb_frames(picsong_ctx *c, int n, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b, size_t frame_stride,
                              int first_iter, int header_mask, uint16_t *d_streams, size_t stream_stride, void *stream)
{
    return encode_rgb_frames_impl(c, n, d_r, d_g, d_b, frame_stride, first_iter, header_mask, d_streams, stream_stride, stream,
                                  "encode_rgb_frames");
}

int picsong_encode_rgb_frame(picsong_ctx *c, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b, int header_mask,
                             uint16_t *d_streams, size_t stream_stride, void *stream)
{
    return encode_rgb_frames_impl(c, 1, d_r, d_g, d_b, 0, 0, header_mask, d_streams, stream_stride, stream, "encode_rgb_frame");
}

// The colour decode calls, their arguments past their refusal: the tables on one coder grid and the batch workspace grown
// to the 3 n planes ...
static int decode_rgb_begin(picsong_ctx *c, int n, BpcArgs &a)
{
    if (int rc = bpc_args_rgb(c, a)) return rc;             // (the tables' geometry)
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_batch(c, 3 * n)) return rc;
    if (int rc = ensure_coef_i(c, 3 * n)) return rc;
    c->last_batch = -1;
    return PICSONG_OK;
}
// ... the fused tails (grid.z = frame), read per call: PICSONG_RGB_NOFUSE=1 keeps the two launches; 9/7: the lean kernel's domain
static bool rgb_tail_switch(const picsong_ctx *c)
{
    if (getenv("PICSONG_RGB_NOFUSE")) return false;
    return !c->p.lossy || !(getenv("PICSONG_DWT_INV97") && atoi(getenv("PICSONG_DWT_INV97")) == 0);
}
// ... then the sequence (decode_rgb_frames, launch_seq.hpp): whole or at 1/2^reduce into the planes d0 .. d2, or win's
// window in `layout`
static int decode_rgb(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, int reduce, const WindowPlan *win, int layout,
                      uint8_t *d0, uint8_t *d1, uint8_t *d2, size_t pitch, size_t frame_stride, void *stream)
{
    BpcArgs a;
    if (int rc = decode_rgb_begin(c, n, a)) return rc;
    return refused_rc(decode_rgb_frames(HipGo{ (hipStream_t)stream }, decode_ctx(c, a, true), a, c->batch, (unsigned)n, d_streams,
                                        stream_stride, reduce, win, dec_c16_reduced(c, reduce), lean97_levels(), rgb_tail_switch(c), layout,
                                        d0, d1, d2, pitch, frame_stride));
}

// picsong_decode_rgb_frames (reduce = 0), picsong_decode_rgb_frames_reduced and their n = 1 forms
static int decode_rgb_frames_impl(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, int reduce, uint8_t *d_r,
                                  uint8_t *d_g, uint8_t *d_b, size_t frame_stride, void *stream, const char *who)
{
    REFUSE_DEEP(c, who);
    if (!c) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    if (const char *why = rgb_frames_reduced_refusal(c->p.is_rgb != 0, c->p.cp, true, n, d_r, d_g, d_b, d_streams, frame_stride, stream_stride,
                                                     picsong_max_stream_shorts(c->aw, c->ah), c->aw, c->ah, c->p.wl, reduce))
        return fail(PICSONG_ERR_ARG, "%s: %s", who, why);
    return decode_rgb(c, n, d_streams, stream_stride, reduce, nullptr, kLayoutPlanar3, d_r, d_g, d_b, 0, frame_stride, stream);
}

int picsong_decode_rgb_frames(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, uint8_t *d_r, uint8_t *d_g,
                              uint8_t *d_b, size_t frame_stride, void *stream)
{
    return decode_rgb_frames_impl(c, n, d_streams, stream_stride, 0, d_r, d_g, d_b, frame_stride, stream, "decode_rgb_frames");
}

int picsong_decode_rgb_frames_reduced(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, int reduce, uint8_t *d_r,
                                      uint8_t *d_g, uint8_t *d_b, size_t frame_stride, void *stream)
{
    return decode_rgb_frames_impl(c, n, d_streams, stream_stride, reduce, d_r, d_g, d_b, frame_stride, stream, "decode_rgb_frames_reduced");
}

int picsong_decode_rgb_frame(picsong_ctx *c, const uint16_t *d_streams, size_t stream_stride, uint8_t *d_r, uint8_t *d_g,
                             uint8_t *d_b, void *stream)
{
    return decode_rgb_frames_impl(c, 1, d_streams, stream_stride, 0, d_r, d_g, d_b, 0, stream, "decode_rgb_frame");
}

int picsong_decode_rgb_frame_reduced(picsong_ctx *c, const uint16_t *d_streams, size_t stream_stride, int reduce, uint8_t *d_r,
                                     uint8_t *d_g, uint8_t *d_b, void *stream)
{
    return decode_rgb_frames_impl(c, 1, d_streams, stream_stride, reduce, d_r, d_g, d_b, 0, stream, "decode_rgb_frame_reduced");
}

// ---------------------------------------------------------------------------------------------
// deep RGB contexts (bit_depth 9..16, components 3, is_rgb 1): n colour frames of three uint16 planes.  Encoding, level 0
// applies the colour transform in its load stage (deep_rgb_forward, launch_seq.hpp; PICSONG_DEEP_NOFUSE=1, read per call: one
// rgb_forward16 launch over the n frames); decoding ends in one rgb_inverse16 launch over the n frames.  Between the ends the
// 3 n planes are deep grey planes: 32-bit coefficients, one launch a stage, plane z with table z % 3.
// ---------------------------------------------------------------------------------------------
#define REFUSE_NOT_DEEP_RGB(c, who)                                                                                      \
    do {                                                                                                                 \
        if ((c) && !is_deep_rgb(c))                                                                                      \
            return fail(PICSONG_ERR_ARG, "%s: uint16 RGB planes want a deep RGB context (bit_depth 9..16, components 3, is_rgb 1)", who); \
    } while (0)

int picsong_rgb_forward16(picsong_ctx *c, const uint16_t *d_r, const uint16_t *d_g, const uint16_t *d_b, void *d_c0, void *d_c1,
                          void *d_c2, void *stream)
{
    REFUSE_NOT_DEEP_RGB(c, "rgb_forward16");
    if (!c || !d_r || !d_g || !d_b || !d_c0 || !d_c1 || !d_c2) return fail(PICSONG_ERR_ARG, "rgb_forward16: null argument");
    if ((((uintptr_t)d_r) | ((uintptr_t)d_g) | ((uintptr_t)d_b)) & 1u)
        return fail(PICSONG_ERR_ARG, "rgb_forward16: uint16 samples need 2-byte aligned pointers");
    if ((((uintptr_t)d_c0) | ((uintptr_t)d_c1) | ((uintptr_t)d_c2)) & 15u)
        return fail(PICSONG_ERR_ARG, "rgb_forward16: the component planes need 16-byte aligned pointers");
    return rgb_forward16(HipGo{ (hipStream_t)stream }, c->p.lossy != 0, d_r, d_g, d_b, d_c0, d_c1, d_c2, c->P / 4, level_off(c));
}

int picsong_rgb_inverse16(picsong_ctx *c, const void *d_c0, const void *d_c1, const void *d_c2, uint16_t *d_r, uint16_t *d_g,
                          uint16_t *d_b, void *stream)
{
    REFUSE_NOT_DEEP_RGB(c, "rgb_inverse16");
    if (!c || !d_r || !d_g || !d_b || !d_c0 || !d_c1 || !d_c2) return fail(PICSONG_ERR_ARG, "rgb_inverse16: null argument");
    if ((((uintptr_t)d_r) | ((uintptr_t)d_g) | ((uintptr_t)d_b)) & 1u)
        return fail(PICSONG_ERR_ARG, "rgb_inverse16: uint16 samples need 2-byte aligned pointers");
    if ((((uintptr_t)d_c0) | ((uintptr_t)d_c1) | ((uintptr_t)d_c2)) & 15u)
        return fail(PICSONG_ERR_ARG, "rgb_inverse16: the component planes need 16-byte aligned pointers");
    return rgb_inverse16(HipGo{ (hipStream_t)stream }, c->p.lossy != 0, d_c0, d_c1, d_c2, d_r, d_g, d_b, c->P / 4, level_off(c), px_max(c));
}

// what the two frame calls refuse alike (nothing launched): rgb_frames_refusal's rules on planes of 2 P bytes, and the
// alignment of 2-byte samples
static int rgb_frames16_args(picsong_ctx *c, int n, const void *r, const void *g, const void *b, const void *streams, size_t frame_stride,
                             size_t stream_stride, const char *who, BpcArgs &a)
{
    REFUSE_NOT_DEEP_RGB(c, who);
    if (!c) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    if (const char *why = rgb_frames_refusal(true, c->p.cp, true, n, r, g, b, streams, frame_stride, stream_stride, 2 * c->P,
                                             picsong_max_stream_shorts(c->aw, c->ah)))
        return fail(PICSONG_ERR_ARG, "%s: %s", who, why);
    if ((((uintptr_t)r) | ((uintptr_t)g) | ((uintptr_t)b) | ((uintptr_t)streams)) & 1u)
        return fail(PICSONG_ERR_ARG, "%s: pointers need 2-byte alignment", who);
    if (n > 1 && (frame_stride & 1u)) return fail(PICSONG_ERR_ARG, "%s: frame_stride %zu must be even", who, frame_stride);
    if (int rc = bpc_args_rgb(c, a)) return rc;             // (the tables' geometry)
    a.frames = 3 * n;
    return PICSONG_OK;
}

int picsong_encode_rgb_frames16(picsong_ctx *c, int n, const uint16_t *d_r, const uint16_t *d_g, const uint16_t *d_b, size_t frame_stride,
                                int first_iter, int header_mask, uint16_t *d_streams, size_t stream_stride, void *stream)
{
    BpcArgs a;
    int rc = rgb_frames16_args(c, n, d_r, d_g, d_b, d_streams, frame_stride, stream_stride, "encode_rgb_frames16", a);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const unsigned np = 3u * (unsigned)n;
    if ((rc = ensure_batch(c, (int)np))) return rc;
    if ((rc = ensure_coef_i(c, (int)np))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t coef_z = (c->P + c->extra) * 4;
    // ---- the levels over the 3 n planes, the colour transform in level 0's load stage (PICSONG_DEEP_NOFUSE=1: one launch of
    // its own, the component planes in batch.coef_i)
    if ((rc = deep_rgb_forward(HipGo{ s }, c->p.lossy != 0, deep_nofuse(), d_r, d_g, d_b, n > 1 ? frame_stride : 0, (unsigned)n, c->batch.coef,
                               c->batch.coef_i, c->aw, c->ah, c->p.wl, c->p.qs, level_off(c), coef_z))) return rc;
    // ---- coder and pack as picsong_encode_rgb_frames, 32-bit coefficients (the header's two depth fields carry bit_depth)
    return rgb_code_and_pack(c, a, n, false, first_iter, header_mask, d_streams, stream_stride, s);
}

int picsong_decode_rgb_frames16(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, uint16_t *d_r, uint16_t *d_g,
                                uint16_t *d_b, size_t frame_stride, void *stream)
{
    BpcArgs a;
    if (int rc = rgb_frames16_args(c, n, d_r, d_g, d_b, d_streams, frame_stride, stream_stride, "decode_rgb_frames16", a)) return rc;
    // (decode_ctx hands the sequence px_max: uint16 samples at d_r / d_g / d_b, frame_stride bytes apart)
    return decode_rgb(c, n, d_streams, stream_stride, 0, nullptr, kLayoutPlanar3, reinterpret_cast<uint8_t *>(d_r),
                      reinterpret_cast<uint8_t *>(d_g), reinterpret_cast<uint8_t *>(d_b), 0, frame_stride, stream);
}

// the window calls, their arguments checked: the window's plan against the decoder's scratch, then the sequence
static int decode_rgb_window_impl(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, int reduce, int x, int y, int w,
                                  int h, int layout, uint8_t *d0, uint8_t *d1, uint8_t *d2, size_t pitch, size_t frame_stride, void *stream,
                                  const char *who)
{
    WindowPlan plan;
    if (int rc = window_args_ok(c, reduce, x, y, w, h, who, &plan)) return rc;
    return decode_rgb(c, n, d_streams, stream_stride, reduce, &plan, layout, d0, d1, d2, pitch, frame_stride, stream);
}

// The proxies of deep RGB frames: picsong_decode_rgb_frames_reduced / _window on uint16 planes, strides and pitch in bytes.
// The same sequence (decode_rgb_frames with DecodeCtx::px_max).  Reduced: the synthesis of the 3 n planes to level
// `reduce`, then ONE rgb_inverse16 launch over the n frames' reduced planes.  Window: level r leaves T samples compact, then
// ONE window_rgb16_image_kernel launch, grid.z = frame.
int picsong_decode_rgb_frames16_reduced(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, int reduce, uint16_t *d_r,
                                        uint16_t *d_g, uint16_t *d_b, size_t frame_stride, void *stream)
{
    const char *who = "decode_rgb_frames16_reduced";
    if (!c) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    if (const char *why = rgb_frames16_reduced_refusal(c->p.bit_depth, c->p.is_rgb != 0, c->p.cp, true, n, d_r, d_g, d_b, d_streams, frame_stride,
                                                       stream_stride, picsong_max_stream_shorts(c->aw, c->ah), c->aw, c->ah, c->p.wl, reduce))
        return fail(PICSONG_ERR_ARG, "%s: %s", who, why);
    return decode_rgb(c, n, d_streams, stream_stride, reduce, nullptr, kLayoutPlanar3_16, reinterpret_cast<uint8_t *>(d_r),
                      reinterpret_cast<uint8_t *>(d_g), reinterpret_cast<uint8_t *>(d_b), 0, frame_stride, stream);
}

int picsong_decode_rgb_frames16_window(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, int reduce, int x, int y,
                                       int w, int h, uint16_t *d_r, uint16_t *d_g, uint16_t *d_b, size_t out_pitch, size_t frame_stride,
                                       void *stream)
{
    const char *who = "decode_rgb_frames16_window";
    if (!c) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    if (const char *why = rgb_frames16_window_refusal(c->p.bit_depth, c->p.is_rgb != 0, c->p.cp, true, n, d_r, d_g, d_b, d_streams, out_pitch,
                                                      frame_stride, stream_stride, picsong_max_stream_shorts(c->aw, c->ah), c->aw, c->ah,
                                                      c->p.wl, reduce, x, y, w, h))
        return fail(PICSONG_ERR_ARG, "%s: %s", who, why);
    return decode_rgb_window_impl(c, n, d_streams, stream_stride, reduce, x, y, w, h, kLayoutPlanar3_16, reinterpret_cast<uint8_t *>(d_r),
                                  reinterpret_cast<uint8_t *>(d_g), reinterpret_cast<uint8_t *>(d_b), out_pitch, frame_stride, stream, who);
}

static int decode_rgb_frames_window_impl(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, int reduce, int x, int y,
                                         int w, int h, uint8_t *d_r, uint8_t *d_g, uint8_t *d_b, size_t out_pitch, size_t frame_stride,
                                         void *stream, const char *who)
{
    REFUSE_DEEP(c, who);
    if (!c) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    if (const char *why = rgb_frames_window_refusal(c->p.is_rgb != 0, c->p.cp, true, n, d_r, d_g, d_b, d_streams, out_pitch, frame_stride,
                                                    stream_stride, picsong_max_stream_shorts(c->aw, c->ah), c->aw, c->ah, c->p.wl, reduce,
                                                    x, y, w, h))
        return fail(PICSONG_ERR_ARG, "%s: %s", who, why);
    return decode_rgb_window_impl(c, n, d_streams, stream_stride, reduce, x, y, w, h, kLayoutPlanar3, d_r, d_g, d_b, out_pitch, frame_stride,
                                  stream, who);
}

int picsong_decode_rgb_frames_window(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, int reduce, int x, int y,
                                     int w, int h, uint8_t *d_r, uint8_t *d_g, uint8_t *d_b, size_t out_pitch, size_t frame_stride,
                                     void *stream)
{
    return decode_rgb_frames_window_impl(c, n, d_streams, stream_stride, reduce, x, y, w, h, d_r, d_g, d_b, out_pitch, frame_stride, stream,
                                         "decode_rgb_frames_window");
}

int picsong_decode_rgb_frame_window(picsong_ctx *c, const uint16_t *d_streams, size_t stream_stride, int reduce, int x, int y,
                                    int w, int h, uint8_t *d_r, uint8_t *d_g, uint8_t *d_b, size_t out_pitch, void *stream)
{
    return decode_rgb_frames_window_impl(c, 1, d_streams, stream_stride, reduce, x, y, w, h, d_r, d_g, d_b, out_pitch, 0, stream,
                                         "decode_rgb_frame_window");
}

static int decode_rgb_images_window_impl(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, int reduce, int x, int y,
                                         int w, int h, const picsong_image *dst, size_t frame_stride, void *stream, const char *who)
{
    // (a deep RGB context takes PLANAR3_16, RGB48 and RGBA64 -- uint16 samples through window_rgb16_image_kernel -- and
    // refuses the 8-bit layouts; a deep grey one has no colour call)
    if (!is_deep_rgb(c)) REFUSE_DEEP(c, who);
    if (const char *why = rgb_images_window_refusal(c->p.is_rgb != 0, c->p.cp, true, n, d_streams, stream_stride,
                                                    picsong_max_stream_shorts(c->aw, c->ah), c->aw, c->ah, c->p.wl, reduce, x, y, w, h,
                                                    dst->layout, dst->data, dst->pitch, dst->plane_stride, frame_stride, is_deep_rgb(c)))
        return fail(PICSONG_ERR_ARG, "%s: %s", who, why);
    uint8_t *const d = (uint8_t *)dst->data;
    return decode_rgb_window_impl(c, n, d_streams, stream_stride, reduce, x, y, w, h, dst->layout, d, d + dst->plane_stride,
                                  d + 2 * dst->plane_stride, dst->pitch, frame_stride, stream, who);
}

int picsong_decode_rgb_images_window(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, int reduce, int x, int y,
                                     int w, int h, const picsong_image *dst, size_t frame_stride, void *stream)
{
    const char *who = "decode_rgb_images_window";
    if (!c || !dst) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    return decode_rgb_images_window_impl(c, n, d_streams, stream_stride, reduce, x, y, w, h, dst, frame_stride, stream, who);
}

// the visible rw x rh pixels at 1/2^reduce.  Two routes, the same bytes: the reduced sequence -- 16-bit
// coefficients, the lean synthesis, the fused tail -- into the context's aligned layout buffer and one emit with the geometry
// (rw, rh, paw, pah), where emit_kernel's group loads fit the reduced rows (reduced_emit_ok); else the window (0, 0, rw, rh)
int picsong_decode_rgb_images_reduced(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, int reduce,
                                      const picsong_image *dst, size_t frame_stride, void *stream)
{
    const char *who = "decode_rgb_images_reduced";
    if (!c || !dst) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    if (!is_deep_rgb(c)) REFUSE_DEEP(c, who);
    if (!reduce_ok(c->p.wl, reduce)) return fail(PICSONG_ERR_ARG, "%s: reduce %d outside 0..%d (wl - 1)", who, reduce, c->p.wl - 1);
    int d[5];
    reduced_dims(c->p.width, c->p.height, c->aw, c->ah, reduce, d);
    // (a deep RGB context: the window route alone -- it decodes no more codeblocks than the reduced sequence and its
    // epilogue writes the layout itself, where the other route would add a uint16 emit pass over planes just written)
    if (is_deep_rgb(c) || !reduced_emit_ok(c->aw, reduce))
        return decode_rgb_images_window_impl(c, n, d_streams, stream_stride, reduce, 0, 0, d[0], d[1], dst, frame_stride, stream, who);
    if (const char *why = rgb_images_window_refusal(c->p.is_rgb != 0, c->p.cp, true, n, d_streams, stream_stride,
                                                    picsong_max_stream_shorts(c->aw, c->ah), c->aw, c->ah, c->p.wl, reduce, 0, 0, d[0], d[1],
                                                    dst->layout, dst->data, dst->pitch, dst->plane_stride, frame_stride))
        return fail(PICSONG_ERR_ARG, "%s: %s", who, why);
    BpcArgs a;
    if (int rc = decode_rgb_begin(c, n, a)) return rc;
    const size_t pp = (size_t)d[2] * (size_t)d[3];
    if (int rc = ensure_layout(c, ((size_t)3 * (size_t)n * pp + c->P - 1) / c->P)) return rc;
    return refused_rc(decode_rgb_images_reduced(HipGo{ (hipStream_t)stream }, decode_ctx(c, a, true), a, c->batch, (unsigned)n, d_streams,
                                                stream_stride, reduce, dec_c16_reduced(c, reduce), lean97_levels(), rgb_tail_switch(c),
                                                c->lay_buf, dst->layout, dst->data, dst->pitch, dst->plane_stride, frame_stride, d[0], d[1]));
}

static int rgb_images_args(picsong_ctx *c, int n, const picsong_image *img, size_t frame_stride, const void *d_streams, size_t stream_stride,
                           const char *who, BpcArgs &a)
{
    if (!c || !img || !d_streams) return fail(PICSONG_ERR_ARG, "%s: null argument", who);
    if (is_deep_rgb(c)) {
        // the 16-bit colour layouts; the padded side is the context's buffer: three uint16 planes a frame, 6 P bytes
        if (n < 1 || n > kRgbMaxFrames) return fail(PICSONG_ERR_ARG, "%s: n outside 1..21", who);
        if (const char *why = layout_refusal(img->layout, img->data, img->pitch, img->plane_stride, frame_stride, img->data, 6 * c->P, n,
                                             c->p.width, c->p.height, c->aw, c->ah, true, true))
            return fail(PICSONG_ERR_ARG, "%s: %s", who, why);
        const uint8_t *stand_in = (const uint8_t *)(uintptr_t)4096;
        return rgb_frames16_args(c, n, stand_in, stand_in + 2 * c->P, stand_in + 4 * c->P, d_streams, 6 * c->P, stream_stride, who, a);
    }
    REFUSE_DEEP(c, who);
    if (const char *why = rgb_images_refusal(img->layout, img->data, img->pitch, img->plane_stride, frame_stride, n, c->p.width, c->p.height,
                                             c->aw, c->ah))
        return fail(PICSONG_ERR_ARG, "%s: %s", who, why);
    // (the padded side is the context's buffer, allocated later: any non-null address P bytes apart stands for its planes)
    const uint8_t *stand_in = (const uint8_t *)(uintptr_t)4096;
    return rgb_frames_args(c, n, stand_in, stand_in + c->P, stand_in + 2 * c->P, d_streams, 3 * c->P, stream_stride, who, a);
}

int picsong_encode_rgb_images(picsong_ctx *c, int n, const picsong_image *src, size_t frame_stride, int first_iter, int header_mask,
                              uint16_t *d_streams, size_t stream_stride, void *stream)
{
    BpcArgs a;
    if (int rc = rgb_images_args(c, n, src, frame_stride, d_streams, stream_stride, "encode_rgb_images", a)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (is_deep_rgb(c)) {
        if (int rc = ensure_layout(c, (size_t)6 * (size_t)n)) return rc;
        if (int rc = ingest_frames(HipGo{ (hipStream_t)stream }, src->layout, src->data, src->pitch, src->plane_stride, frame_stride, c->lay_buf,
                                   6 * c->P, n, c->p.width, c->p.height, c->aw, c->ah, nullptr, px_max(c))) return rc;
        const uint16_t *const lay = reinterpret_cast<const uint16_t *>(c->lay_buf);
        return picsong_encode_rgb_frames16(c, n, lay, lay + c->P, lay + 2 * c->P, 6 * c->P, first_iter, header_mask, d_streams, stream_stride, stream);
    }
    if (int rc = ensure_layout(c, (size_t)3 * (size_t)n)) return rc;
    if (int rc = ingest_frames(HipGo{ (hipStream_t)stream }, src->layout, src->data, src->pitch, src->plane_stride, frame_stride, c->lay_buf,
                               3 * c->P, n, c->p.width, c->p.height, c->aw, c->ah)) return rc;
    return picsong_encode_rgb_frames(c, n, c->lay_buf, c->lay_buf + c->P, c->lay_buf + 2 * c->P, 3 * c->P, first_iter, header_mask, d_streams,
                                     stream_stride, stream);
}

int picsong_decode_rgb_images(picsong_ctx *c, int n, const uint16_t *d_streams, size_t stream_stride, const picsong_image *dst,
                              size_t frame_stride, void *stream)
{
    BpcArgs a;
    if (int rc = rgb_images_args(c, n, dst, frame_stride, d_streams, stream_stride, "decode_rgb_images", a)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (is_deep_rgb(c)) {
        if (int rc = ensure_layout(c, (size_t)6 * (size_t)n)) return rc;
        uint16_t *const lay = reinterpret_cast<uint16_t *>(c->lay_buf);
        if (int rc = picsong_decode_rgb_frames16(c, n, d_streams, stream_stride, lay, lay + c->P, lay + 2 * c->P, 6 * c->P, stream)) return rc;
        return emit_frames(HipGo{ (hipStream_t)stream }, dst->layout, c->lay_buf, 6 * c->P, dst->data, dst->pitch, dst->plane_stride, frame_stride,
                           n, c->p.width, c->p.height, c->aw, c->ah, nullptr, px_max(c));
    }
    if (int rc = ensure_layout(c, (size_t)3 * (size_t)n)) return rc;
    if (int rc = picsong_decode_rgb_frames(c, n, d_streams, stream_stride, c->lay_buf, c->lay_buf + c->P, c->lay_buf + 2 * c->P, 3 * c->P,
                                           stream)) return rc;
    return emit_frames(HipGo{ (hipStream_t)stream }, dst->layout, c->lay_buf, 3 * c->P, dst->data, dst->pitch, dst->plane_stride, frame_stride,
                       n, c->p.width, c->p.height, c->aw, c->ah);
}

int picsong_pad_frame_host(const uint8_t *in, int w, int h, uint8_t *out, int aw, int ah)
{
    if (!in || !out || w <= 0 || h <= 0 || aw < w || ah < h) return fail(PICSONG_ERR_ARG, "pad_frame: bad argument");
    // column w + j mirrors column w - 1 - j, row h + r mirrors row h - 1 - r: with more added columns
    // (rows) than columns (rows) the reference's loop indexes before its vector's begin
    // (IO/IOManager.ipp:101-108, undefined behaviour on row 0) -- refused here
    if (aw - w > w || ah - h > h)
        return fail(PICSONG_ERR_ARG, "pad_frame: %dx%d -> %dx%d adds more columns/rows than the frame has", w, h, aw, ah);
    for (int y = 0; y < h; y++) {
        memcpy(out + (size_t)y * aw, in + (size_t)y * w, (size_t)w);
        for (int j = 0; j < aw - w; j++) out[(size_t)y * aw + w + j] = in[(size_t)y * w + (w - 1 - j)];
    }
    for (int r = 0; r < ah - h; r++) memcpy(out + (size_t)(h + r) * aw, out + (size_t)(h - 1 - r) * aw, (size_t)aw);
    return PICSONG_OK;
}

// the same rule on 2-byte samples
int picsong_pad_frame16_host(const uint16_t *in, int w, int h, uint16_t *out, int aw, int ah)
{
    if (!in || !out || w <= 0 || h <= 0 || aw < w || ah < h) return fail(PICSONG_ERR_ARG, "pad_frame16: bad argument");
    if (aw - w > w || ah - h > h)
        return fail(PICSONG_ERR_ARG, "pad_frame16: %dx%d -> %dx%d adds more columns/rows than the frame has", w, h, aw, ah);
    for (int y = 0; y < h; y++) {
        memcpy(out + (size_t)y * aw, in + (size_t)y * w, (size_t)w * 2);
        for (int j = 0; j < aw - w; j++) out[(size_t)y * aw + w + j] = in[(size_t)y * w + (w - 1 - j)];
    }
    for (int r = 0; r < ah - h; r++) memcpy(out + (size_t)(h + r) * aw, out + (size_t)(h - 1 - r) * aw, (size_t)aw * 2);
    return PICSONG_OK;
}

}  // extern "C"

#ifdef PICSONG_DWT_TRACE
// variant builds only (tools/dwt_trace.py): device buffer the fused DWT head's waves stamp their phases into
extern "C" int picsong_debug_set_trace(void *d_buf)
{
    unsigned long long *p = (unsigned long long *)d_buf;
    return hipMemcpyToSymbol(HIP_SYMBOL(picsong::g_dwt_trace), &p, sizeof p) == hipSuccess ? 0 : -1;
}
extern "C" int picsong_debug_set_bpc_trace(void *d_buf)
{
    unsigned long long *p = (unsigned long long *)d_buf;
    return hipMemcpyToSymbol(HIP_SYMBOL(picsong::g_bpc_trace), &p, sizeof p) == hipSuccess ? 0 : -1;
}
#endif
