/*
 * picsong_hip.h -- C ABI of the MI355X-native PICSONG hot path
 *                  (level shift -> DWT 5/3 | 9/7 -> BPC-PaCo -> BitStreamBuilder, and inverse).
 *
 * The reference (13Karl/CUDA-Image-and-Video-codec) exposes no FFI; the seam this library replaces
 * is the C++ facade layer its engines call with device pointers and a stream.
 * Each entry point cites the reference interface it stands in for (paths relative to
 * CUDA_ImCod/).  Conventions:
 *   - plain C linkage, POD arguments, caller-owned device memory, no torch / C++ types;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - every function returns PICSONG_OK (0) or a negative error code; nothing calls exit()
 *     (the reference prints and exits, SupportFunctions/AuxiliarFunctions.cpp:39-56);
 *     picsong_last_error() returns a thread-local message for the last failure;
 *   - stage functions are asynchronous on `stream` unless their name ends in _sync or they
 *     return a host value (documented per function);
 *   - a context is thread-safe for concurrent use only with distinct workspaces/streams, as the
 *     reference's facades are (one set of scratch buffers per worker, CodingEngine.cu:157-197).
 */
#ifndef PICSONG_HIP_H
#define PICSONG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PICSONG_OK 0
#define PICSONG_ERR_ARG (-1)        /* invalid argument / validity limit of SURVEY A.9 */
#define PICSONG_ERR_HIP (-2)        /* a HIP runtime call failed */
#define PICSONG_ERR_IO (-3)         /* LUT folder / file problem */
#define PICSONG_ERR_NOMEM (-4)
#define PICSONG_ERR_RANGE (-5)      /* a codeblock exceeded the supported magnitude range */
#define PICSONG_ERR_NODEVICE (-6)   /* no usable GPU: the product has no CPU fallback */
#define PICSONG_ERR_RATE (-7)       /* no quantiser of the search range meets the target size */
#define PICSONG_ERR_QUALITY (-8)    /* no quantiser of the search range meets the distortion limit */

#define PICSONG_CB 64               /* codeblock edge, BPC/BPCEngine.cuh:29-36 */
#define PICSONG_CB_WORDS 4096       /* staging ints per codeblock */
#define PICSONG_HDR_SHORTS 9        /* global header, BitStreamBuilder.cpp:54-93 */

/* Coding parameters == the flag globals of Launcher.cu:8-29 that reach the hot path. */
typedef struct picsong_params {
    int width, height;      /* -xSize / -ySize (unpadded) */
    int wl;                 /* -wl, 1..7 (header limit) */
    int cp;                 /* -cp: 2 coding passes, or 3 (deprecated in the reference; needs the cp_sig / cp_sign tables) */
    int lossy;              /* -type: 0 = 5/3 reversible, 1 = 9/7 + quantisation */
    float qs;               /* -qs */
    float k;                /* -k: 0 = two coding passes on every plane; > 0 = complexity-scalable bulk mode */
    int cb_width, cb_height;/* -cbWidth / -cbHeight: header-only */
    int bit_depth;          /* -bps (8) */
    int frames;             /* -frames (header only) */
    int components;         /* -components: 1 (grey) or 3 (with is_rgb) */
    int is_rgb;             /* -isRGB: planar R,G,B planes, RCT (lossless) / ICT (lossy) colour transform */
} picsong_params;

/* LUT geometry == header.txt (Engines/Engine.cu:190-210) + section sizes
 * (IO/IOManager.ipp:431-433). */
typedef struct picsong_lut_info {
    int n_bitplanes, n_subbands, ctx_ref, ctx_sign, ctx_sig, precision, n_files, n_bp_files;
    int n_ref, n_sig, n_sign;       /* section sizes in ints; table = [ref | sig | sign] */
    int n_tables;                   /* tables laid back to back: 1 (k = 0, file _0) or the bit-plane
                                     * files _0.._(n-1) of -k > 0 (Engines/Engine.cu:12-56); 0 == 1 */
    int cp;                         /* coding passes the table is laid out for: 2 (or 0) = [ref | sig | sign];
                                     * 3 = that followed by [cp_sig | cp_sign] (IO/IOManager.ipp:539-606) */
} picsong_lut_info;

typedef struct picsong_ctx picsong_ctx;

const char *picsong_last_error(void);
const char *picsong_version(void);

/* ---- geometry (SupportFunctions/AuxiliarFunctions.cpp:22-26, CodingEngine.cu:170-177) ---- */
int    picsong_pad_dim(int v);
size_t picsong_dwt_extra(int aw, int ah, int wl);
/* upper bound of one frame's codestream in shorts: 9 + 2 nCB + AW*AH + 1 */
size_t picsong_max_stream_shorts(int aw, int ah);

/* ---- header (BitStreamBuilder::setExtraInformation BitStreamBuilder.cpp:35-94 <->
 *      DecodingEngine::getExtraInformation Engines/DecodingEngine.cu:567-585), host only ---- */
int picsong_header_pack(const picsong_params *p, uint16_t out[PICSONG_HDR_SHORTS]);
int picsong_header_unpack(const uint16_t in[PICSONG_HDR_SHORTS], picsong_params *p);

/* ---- LUT text parser (IOManager::loadLUTHeaders IO/IOManager.ipp:363-386 +
 *      IOManager::loadLUTUpgraded :404-612), host only.  component 1/2/3 = R/G/B files,
 *      0 = un-suffixed.  `fill` = value of entries the reference never writes (de-facto 0,
 *      SURVEY fact 5).  table may be NULL to query info->n_* first. ---- */
int picsong_lut_load(const char *folder, int component, int wl, int fill,
                     picsong_lut_info *info, int32_t *table, size_t table_capacity);
/* -k > 0 (Engine::initLUT's multi-file branch, Engines/Engine.cu:12-56): the tables of files
 * _0 .. _(n_tables-1), table j at offset j * (n_ref + n_sig + n_sign); n_tables <= 0 = all
 * AMOUNT_OF_BITPLANE_FILES.  table needs n_tables * (n_ref + n_sig + n_sign) ints
 * (query with table == NULL: info->n_tables is filled in). */
int picsong_lut_load_k(const char *folder, int component, int wl, int fill, int n_tables,
                       picsong_lut_info *info, int32_t *table, size_t table_capacity);

/* -cp 3 (Engine::initLUT with codingPasses == 3, Engines/Engine.cu:56-100; loader IO/IOManager.ipp:539-606):
 * file _0 of ref, sig, sign, cp_sig and cp_sign; table needs n_ref + 2 (n_sig + n_sign) ints.  cp = 2 is
 * picsong_lut_load. */
int picsong_lut_load_cp(const char *folder, int component, int wl, int fill, int cp,
                        picsong_lut_info *info, int32_t *table, size_t table_capacity);

/* ---- context: replaces `new DWT<T,Y>(...)` / `new BPCCuda<T>(...)` + Engine::initLUT's
 *      cudaMalloc/cudaMemcpy of the table (Engines/Engine.cu:111-136).  Owns only the LUT copy
 *      and a small internal workspace (scan scratch, flags, the frame pipeline's buffers when
 *      picsong_encode_frame/picsong_decode_frame are used). ---- */
int  picsong_ctx_create(const picsong_params *p, int device, picsong_ctx **out);
void picsong_ctx_destroy(picsong_ctx *ctx);
int  picsong_ctx_set_lut(picsong_ctx *ctx, const picsong_lut_info *info, const int32_t *host_table);
int  picsong_ctx_padded_dims(const picsong_ctx *ctx, int *aw, int *ah, int *n_codeblocks);
/* Hint, no effect on results: on != 0 says that frames of OTHER contexts / streams are in flight on
 * this GPU while this context's frames run (the reference's -numberOfStreams > 1 video engine,
 * Engines/CodingEngine.cu:758-1069): throughput over latency.  What it selects today: the -k > 0 encoder's
 * instantiation (six waves a SIMD with compact table copies when hinted, the register-rich four-wave one for a
 * lone frame).  The k = 0 kernels take the same launches either way -- their waves ask for issue priority by
 * plane count instead, which serves a lone frame and costs frames in flight nothing.  Default: off. */
int  picsong_ctx_set_pipelined(picsong_ctx *ctx, int on);
/* RGB: component c (0,1,2) uses its own table, files {ref,sig,sign}{R,G,B}.txt_0
 * (Engine::initLUT Engines/Engine.cu:124-136: _LUTInformation[i]); picsong_ctx_set_lut == component 0.
 * Both setters refuse (PICSONG_ERR_ARG, the context keeps the table it held) a table whose geometry the coders cannot
 * read as the whole array clamps it: several tables (n_tables > 1) on a k = 0 or -cp 3 context, which codes with one;
 * and on a -k > 0 context, sections that leave the furthest index the coders form -- bit-plane 15 of the highest
 * subband group, max(wl * n_subbands, (wl - 1) * n_subbands + 2) -- more than 16 entries past one table (with three
 * subbands and sections sized for the context's wl: n_bitplanes < 12). */
int  picsong_ctx_set_lut_component(picsong_ctx *ctx, int component, const picsong_lut_info *info,
                                   const int32_t *host_table);

/* The reference hands BPCCuda<T>::Code / Decode the DEVICE copy of the table with its geometry on every call
 * (`int* LUTInformation` + six integers, BPC/BPCEngine.hpp:16-17; Engine::initLUT made that copy,
 * Engines/Engine.cu:111-136).  This adopts such a caller-owned device table for component slot c without
 * copying it: it must stay valid while the context uses it.  info->n_ref / n_sig / n_sign == 0 are derived
 * from the geometry and the context's wl (IO/IOManager.ipp:431-433).
 * The k = 0 encoder codes from an image of per-(subband group, bit-plane) records of the table.  For a host table the
 * setter builds it once; for a table adopted here one small block rebuilds it from the table ahead of every encoder
 * launch, on that launch's stream, so the entries may change between calls as they always could. */
int  picsong_ctx_set_lut_device(picsong_ctx *ctx, int component, const picsong_lut_info *info,
                                const int32_t *d_table);

/* ---- level shift: offsetImage<T> Engines/CodingEngine.cu:581-588 and
 *      removeOffsetAndApplyMaxMin(/Lossy) Engines/DecodingEngine.cu:706-729.
 *      T = int32 (lossless ctx) or float (lossy ctx); n = AW*AH. ---- */
int picsong_level_shift_fwd(picsong_ctx *ctx, const uint8_t *d_in, void *d_out, void *stream);
int picsong_level_shift_inv(picsong_ctx *ctx, void *d_data, void *stream);

/* ---- DWT: DWT<T,Y>::DWTEncode(T* in, T* out, stream) / DWTDecode(int* in, T* out, stream)
 *      (DWT/DWTGenerator.hpp:27-29, DWT/DWTGenerator.cu:1268-1424).  Same buffer contract:
 *      d_out has AW*AH + picsong_dwt_extra() elements; forward leaves the Mallat-layout
 *      coefficients (row stride AW) in d_out[0 .. AW*AH); inverse leaves the image at
 *      d_out + picsong_dwt_extra().  Quantisation / de-quantisation fused for lossy. ---- */
int picsong_dwt_forward(picsong_ctx *ctx, const void *d_in, void *d_out, void *stream);
int picsong_dwt_inverse(picsong_ctx *ctx, const int32_t *d_in, void *d_out, void *stream);
/* level-0 u8 ingest with the level shift fused (the reference's deprecated DWTEncodeChar,
 * DWT/DWTGenerator.cu:1141-1261, is the model); results identical to shift + forward. */
int picsong_dwt_forward_u8(picsong_ctx *ctx, const uint8_t *d_in, void *d_out, void *stream);

/* ---- BPC: BPCEngine<T>::kernelLauncher(CODE|DECODE) BPC/BPCEngine.cu:2307-2424 preceded by
 *      deviceMemoryAllocator's 0xFF memset (:2429-2441).  d_coeffs: Mallat T[AW*AH];
 *      d_staging: int32[AW*AH] (4096 per codeblock: [0] = MSB, [1..len) codewords);
 *      d_sizes: int32[nCB].  (The encoders themselves keep a 16-bit staging -- no staging word holds more
 *      than 16 bits -- in a buffer of the context; picsong_bpc_encode fills d_staging with 0xFF bytes and
 *      widens words [0, len) of every codeblock into it: the array a caller sees is the reference's.) ---- */
int picsong_bpc_encode(picsong_ctx *ctx, const void *d_coeffs, int32_t *d_staging,
                       int32_t *d_sizes, void *stream);
int picsong_bpc_decode(picsong_ctx *ctx, const int32_t *d_staging, const int32_t *d_sizes,
                       int32_t *d_coeffs, void *stream);

/* the same with the table of component slot 0..2 (RGB: the reference passes _LUTInformation[i],
 * Engines/CodingEngine.cu:617, Engines/DecodingEngine.cu:799-823) */
int picsong_bpc_encode_component(picsong_ctx *ctx, int component, const void *d_coeffs, int32_t *d_staging,
                                 int32_t *d_sizes, void *stream);
int picsong_bpc_decode_component(picsong_ctx *ctx, int component, const int32_t *d_staging,
                                 const int32_t *d_sizes, int32_t *d_coeffs, void *stream);

/* ---- BitStreamBuilder: createBitStream BitStreamBuilder.cpp:100-114 (CUB InclusiveSum +
 *      index LUT + buildBitStreamLUTBS BitStreamBuilder.cu:106-137,290-323) and createCodeStream
 *      BitStreamBuilder.cpp:134-153.  h_header NULL == iter != 0 (header shorts stay 0xFFFF).
 *      pack: *h_total (host) receives the stream length in shorts after an internal stream
 *      synchronisation, exactly like HTotalBSSize[0]; pass NULL to stay asynchronous and read
 *      the length later with picsong_last_total(). ---- */
int picsong_bitstream_pack(picsong_ctx *ctx, const int32_t *d_staging, const int32_t *d_sizes,
                           const uint16_t *h_header, uint16_t *d_stream, int *h_total,
                           void *stream);
int picsong_bitstream_unpack(picsong_ctx *ctx, const uint16_t *d_stream, int32_t *d_staging,
                             int32_t *d_sizes, void *stream);
/* synchronises `stream` and returns the total (shorts) of the most recent pack on this ctx */
int picsong_last_total(picsong_ctx *ctx, void *stream, int *h_total);

/* ---- whole frame: the grey call sequences of CodingEngine::runImage/runVideo
 *      (Engines/CodingEngine.cu:634-674,819-872) and DecodingEngine::runImage
 *      (Engines/DecodingEngine.cu:770-794).  d_frame: padded u8[AW*AH] (caller pads as
 *      IOManager::loadFrameCAdaptedSizes does, uses picsong_pad_frame_host, or has picsong_ingest_frames make it on
 *      the device from the unpadded frame; picsong_encode_images takes that frame directly).  iter == 0
 *      writes the populated header.  Asynchronous; length via picsong_last_total().
 *      picsong_decode_frame reads the stream's own shorts and nothing beyond them (-cp 2: the coder
 *      takes its codewords from d_stream itself; -cp 3 through the staging, as
 *      picsong_bitstream_unpack does); lengths outside 1..4096 are clamped and raise the range flag.  A
 *      DAMAGED length table can still claim more codewords than the stream holds: reads then reach up to
 *      picsong_max_stream_shorts() shorts, so an untrusted stream belongs in a buffer of that size (as with
 *      picsong_bitstream_unpack).
 *      Alignment: none required of d_frame.  A 16-byte aligned frame (what an allocator returns) takes the vector
 *      kernels and the 16-bit coefficient form; any other pointer -- a view at an odd offset -- takes the per-column
 *      kernels with the 32-bit arrays: same codestream, slower. ---- */
int picsong_encode_frame(picsong_ctx *ctx, const uint8_t *d_frame, int iter, uint16_t *d_stream,
                         void *stream);
int picsong_decode_frame(picsong_ctx *ctx, const uint16_t *d_stream, uint8_t *d_frame_out,
                         void *stream);
/* ---- batched frames: n consecutive frames of a video through ONE launch per stage (grid.z = frame for the
 *      DWT levels, one coder grid over n x nCB codeblocks, one pack grid) -- CodingEngine::runVideo's call
 *      sequence (Engines/CodingEngine.cu:819-872) for frames first_iter .. first_iter + n - 1, which the
 *      reference spreads over -numberOfStreams worker threads (:990-1061).  Frame f is the padded
 *      u8[AW*AH] at d_frames + f * frame_stride (bytes, 16-byte aligned), its codestream lands at
 *      d_streams + f * stream_stride (shorts, >= picsong_max_stream_shorts); only the video's frame 0
 *      (first_iter + f == 0) carries the populated header.  n = 1..64; the context grows its workspace to
 *      the largest n seen (about 10 bytes per pixel per frame).  Asynchronous; picsong_last_totals
 *      synchronises `stream` and returns the n lengths in shorts.  Byte-identical to n calls of
 *      picsong_encode_frame.  Grey -cp 2 contexts, any -k (k > 0: the BULK coder instantiations over the
 *      n frames of the launch); -cp 3 is coded frame by frame. ---- */
int picsong_encode_frames(picsong_ctx *ctx, int n, const uint8_t *d_frames, size_t frame_stride, int first_iter,
                          uint16_t *d_streams, size_t stream_stride, void *stream);
int picsong_last_totals(picsong_ctx *ctx, void *stream, int n, int *h_totals);
/* The mirror for decoding: n codestreams (stream f at d_streams + f * stream_stride shorts) to n padded u8 frames (frame f
 * at d_frames_out + f * frame_stride bytes, 4-byte aligned strides) through one launch per stage -- DecodingEngine's
 * video loop (Engines/DecodingEngine.cu:734-1141) for n consecutive frames.  Byte-identical to n calls of
 * picsong_decode_frame; grey -cp 2 contexts, any -k. */
int picsong_decode_frames(picsong_ctx *ctx, int n, const uint16_t *d_streams, size_t stream_stride, uint8_t *d_frames_out,
                          size_t frame_stride, void *stream);
/* The same lengths without a wait: copies the totals of the most recent picsong_encode_frame (n = 1) or
 * picsong_encode_frames (n = its frame count) into d_totals (device, int32[n]) on `stream`.  A caller that keeps
 * many calls in flight (the frame-sharded multi-GPU exchange, bench.py --gpus N) collects them per bucket of
 * calls and reads them back once, instead of synchronising after every call. */
int picsong_copy_last_totals(picsong_ctx *ctx, void *stream, int n, int32_t *d_totals);

/* ---- RGB path: RGBTransformLossless / RGBTransformLossy with the level shift
 *      fused (Engines/CodingEngine.cu:357-403,408-449; Engines/DecodingEngine.cu:599-701), then each
 *      component is coded as a frame of its own with its own LUT (CodingEngine.cu:598-633,676-712).
 *      Planes are padded AW*AH arrays; T = int32 (lossless ctx) or float (lossy ctx).
 *      encode_plane = DWTEncode + Code for one component; with_header == the reference's iter == 0.
 *      decode_plane = Decode + DWTDecode: d_plane_out has AW*AH + picsong_dwt_extra() elements, the
 *      component lands at d_plane_out + extra (no clamp: the inverse colour transform clamps). ---- */
int picsong_rgb_forward(picsong_ctx *ctx, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b,
                        void *d_c0, void *d_c1, void *d_c2, void *stream);
int picsong_rgb_inverse(picsong_ctx *ctx, const void *d_c0, const void *d_c1, const void *d_c2,
                        uint8_t *d_r, uint8_t *d_g, uint8_t *d_b, void *stream);
int picsong_encode_plane(picsong_ctx *ctx, const void *d_plane, int component, int with_header,
                         uint16_t *d_stream, void *stream);
int picsong_decode_plane(picsong_ctx *ctx, const uint16_t *d_stream, int component, void *d_plane_out,
                         void *stream);
/* One RGB frame through ONE launch per stage -- the colour transform, then its three components as the three frames
 * of the batched grid: grid.z = 3 for the transform's levels, one coder grid in which component c codes with table c,
 * one scan + pack -- in place of picsong_rgb_forward + 3 x picsong_encode_plane (the reference codes the components
 * one after the other, Engines/CodingEngine.cu:598-633).  d_r / d_g / d_b: padded u8[AW*AH] planes; component c's
 * codestream lands at d_streams + c * stream_stride (shorts, >= picsong_max_stream_shorts); header_mask bit c = that
 * component carries the populated header (image: 1 -- component 0 only, iter = component; video frame 0: 7; else 0).
 * Lengths: picsong_last_totals(ctx, stream, 3, ..) / picsong_copy_last_totals.  Byte-identical to the plane-by-plane
 * calls; -cp 2 RGB contexts (any -k) whose three tables share one geometry.  The planes need 4-byte alignment; the
 * fused head (the colour transform, RCT or ICT, in the transform's load stage) runs when all three are 16-byte
 * aligned, the separate colour-transform kernel otherwise (same streams).  The decoder's mirror takes the three
 * codestreams (same stride) to the three padded u8 planes (Engines/DecodingEngine.cu:599-701, 736-769); its 5/3 form
 * runs the inverse colour transform inside the finest synthesis level. */
int picsong_encode_rgb_frame(picsong_ctx *ctx, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b, int header_mask,
                             uint16_t *d_streams, size_t stream_stride, void *stream);
int picsong_decode_rgb_frame(picsong_ctx *ctx, const uint16_t *d_streams, size_t stream_stride, uint8_t *d_r, uint8_t *d_g,
                             uint8_t *d_b, void *stream);

/* ---- reduced-resolution decode (JPEG 2000's resolution reduction, OpenJPEG -r / Kakadu -reduce; the reference has no
 *      counterpart): the image at 1/2^reduce of the frame's size, for thumbnails, previews and editing proxies.  It is
 *      LL_reduce, the intermediate the full synthesis makes on its way to level 0, level-shifted and clamped as the
 *      full decode's pixels are (5/3: clamp(v + 128); 9/7: rint(v + 128 + 0.01), clamped) -- the low-pass filters have
 *      DC gain 1.  Only the codeblocks that meet the corner [0, AW >> reduce) x [0, AH >> reduce) of the Mallat array
 *      (the subbands of levels reduce + 1 .. wl and LL_wl) are read and decoded, and only the synthesis levels
 *      wl - 1 .. reduce run.  reduce = 0 is the full decode, byte-identical to the calls above; reduce = wl (the coded
 *      LL band itself) is refused.
 *      picsong_reduced_dims: rw x rh = ceil(W / 2^reduce) x ceil(H / 2^reduce), the visible part; paw x pah =
 *      (AW >> reduce) x (AH >> reduce), what the calls write; n_codeblocks = ceil(paw / 64) * ceil(pah / 64), the
 *      codeblocks a call decodes (per frame, per component).
 *      The calls write exactly paw * pah bytes a frame (a plane), row stride paw, and no byte beyond them.  Refused
 *      (PICSONG_ERR_ARG, nothing launched): reduce outside 0..wl - 1, -cp 3 contexts, null pointers, and the stride
 *      checks of the full-size calls (frame_stride >= paw * pah).  Alignment as picsong_decode_frame: a 4-byte
 *      aligned output takes the fused pixel store, any other pointer a separate clamp over paw * pah samples; same
 *      bytes.  picsong_range_flag covers the codeblocks a call decodes (and every length of the stream).
 *      picsong_decode_frames_reduced: the batched mirror of picsong_decode_frames (n = 1..64, one launch per stage;
 *      byte-identical to n calls of picsong_decode_frame_reduced).  picsong_decode_rgb_frame_reduced: the mirror of
 *      picsong_decode_rgb_frame, the inverse RCT / ICT applied to the three components' LL_reduce. ---- */
int picsong_reduced_dims(const picsong_ctx *ctx, int reduce, int *rw, int *rh, int *paw, int *pah, int *n_codeblocks);
int picsong_decode_frame_reduced(picsong_ctx *ctx, const uint16_t *d_stream, int reduce, uint8_t *d_out, void *stream);
int picsong_decode_frames_reduced(picsong_ctx *ctx, int n, const uint16_t *d_streams, size_t stream_stride, int reduce,
                                  uint8_t *d_frames_out, size_t frame_stride, void *stream);
int picsong_decode_rgb_frame_reduced(picsong_ctx *ctx, const uint16_t *d_streams, size_t stream_stride, int reduce,
                                     uint8_t *d_r, uint8_t *d_g, uint8_t *d_b, void *stream);

/* ---- window decode (JPEG 2000 style spatial random access, OpenJPEG -d / Kakadu -region; the reference has no
 *      counterpart): the rectangle [x, x + w) x [y, y + h) of the padded image at 1/2^reduce resolution (the paw x pah
 *      of picsong_reduced_dims), byte for byte that rectangle of picsong_decode_frame_reduced's output, decoded from
 *      only the codeblocks it depends on.  Per synthesis level l = reduce .. wl - 1 the rectangle R_l of LL_l needs the
 *      subband rectangle S_l = [max(0, floor(a / 2) - e), min(K, ceil(b / 2) + e)) per axis ([a, b) = R_l, K the
 *      subband size, e = 1 for 5/3, 2 for 9/7), R_{l+1} = S_l; the call decodes the codeblocks that meet S_l in HL, LH
 *      and HH of every such level and S_{wl-1} as LL_wl, and computes only that cone of the synthesis.
 *      Row i of the window goes to d_out + i * out_pitch, w bytes; nothing else is written (not the gap between rows,
 *      not past the last row); any alignment.  picsong_decode_frames_window: frame f at d_out + f * frame_stride,
 *      byte-identical to n calls of picsong_decode_frame_window (n = 1..64, one launch per stage).
 *      picsong_decode_rgb_frame_window: the inverse RCT / ICT of the three components' windows, the three planes with
 *      the same pitch.  picsong_window_codeblocks: the codeblocks one call decodes (per frame, per component).
 *      Refused (PICSONG_ERR_ARG, nothing launched): reduce outside 0..wl - 1, w < 1 or h < 1, a window not inside
 *      paw x pah, out_pitch < w, frame_stride < (h - 1) * out_pitch + w (n > 1), the stream-stride and n checks of the
 *      reduced calls, null pointers, -cp 3 contexts.  picsong_range_flag covers the codeblocks a call decodes (and
 *      every length of the stream). ---- */
int picsong_window_codeblocks(const picsong_ctx *ctx, int reduce, int x, int y, int w, int h, int *n_codeblocks);
int picsong_decode_frame_window(picsong_ctx *ctx, const uint16_t *d_stream, int reduce, int x, int y, int w, int h,
                                uint8_t *d_out, size_t out_pitch, void *stream);
int picsong_decode_frames_window(picsong_ctx *ctx, int n, const uint16_t *d_streams, size_t stream_stride, int reduce,
                                 int x, int y, int w, int h, uint8_t *d_out, size_t out_pitch, size_t frame_stride,
                                 void *stream);
int picsong_decode_rgb_frame_window(picsong_ctx *ctx, const uint16_t *d_streams, size_t stream_stride, int reduce,
                                    int x, int y, int w, int h, uint8_t *d_r, uint8_t *d_g, uint8_t *d_b,
                                    size_t out_pitch, void *stream);

/* ---- reduced-quality decode (JPEG 2000's quality layers, OpenJPEG -l / Kakadu -layers; the reference has no
 *      counterpart): the frame at its full size from fewer bit-planes, the third way to decode less than the whole
 *      frame beside `reduce` and the window, and it composes with both.  A context carries a decode setting `drop`,
 *      0..15, default 0.  A codeblock's codewords are coded plane after plane from its MSB down, so stopping early reads
 *      a prefix of them and runs a prefix of the coder's work -- and the lowest planes are the expensive ones.
 *      Planes dropped: codeblock cb of the padded Mallat array (raster index, 64 x 64) has the level of its top-left
 *      sample -- 0 the finest detail level, wl the LL band -- and drops d(cb) = max(0, drop - level(cb)) planes: one
 *      plane more a level finer, about the growth of a coefficient's weight in the image per synthesis level (the same
 *      count in every subband costs ~5 dB more at the same drop).  One d a codeblock, also where a subband's width is no
 *      multiple of 64 and the codeblock's columns lie in two subbands.  picsong_drop_planes gives d(cb) on the host, no
 *      context needed.
 *      A coded codeblock decodes its planes MSB .. d exactly as ever; planes d - 1 .. 0 are neither read nor decoded.
 *      Every coefficient that became significant in the decoded planes gets its sign and the magnitude
 *      (m >> d << d) | (1 << (d - 1)), its decoded bits and the midpoint of the interval they leave (JPEG 2000's
 *      r = 1/2) for d >= 1; every other coefficient is 0.  MSB < d: the codeblock is all zero.  Raw codeblocks (the
 *      expansion fallback, length 4096) hold words, not planes: copied whole.  All-zero codeblocks as ever.  An MSB > 15
 *      still raises the range flag.  The midpoint sets no bit above a coefficient's own MSB: the int16 coefficient form
 *      stays within its bound.
 *      Everything after the coder is unchanged -- the de-quantisation and the synthesis run on these coefficients -- so a
 *      reduced or window call under `drop` returns the LL_reduce, or the rectangle, that the full-size call under the
 *      same `drop` computes on its way.
 *      The setting applies to every decoder launch of the context from then on: picsong_bpc_decode(_component),
 *      picsong_decode_plane and every frame decode call (single, n frames, _reduced, _window, grey, RGB -- the same drop
 *      for the three components -- and the picsong_image forms).  Encoding, training and the rate / quality searches
 *      ignore it: a quality search measures the full decode.  drop = 0 is the plain decode in every respect, the kernels
 *      launched included; the setting is plain state, 0 after any value restores the plain decode.
 *      Refused (PICSONG_ERR_ARG, the setting kept): drop outside 0..15; a -k > 0 context (its planes below cbp are the
 *      bulk scan's) and a -cp 3 context (a plane in three passes): both code the low planes differently.
 *      picsong_drop_planes refuses aw / ah that are no positive multiples of 64, wl outside 1..7, drop outside 0..15 and
 *      cb outside the raster. ---- */
int picsong_ctx_set_decode_drop(picsong_ctx *ctx, int drop);
int picsong_ctx_get_decode_drop(const picsong_ctx *ctx, int *drop);
int picsong_drop_planes(int aw, int ah, int wl, int drop, int cb, int *planes);

/* ---- training: probability tables from a corpus (the reference ships four trained folders and no way to make one).
 *      The coder adapts nothing at run time: every binary decision is coded with the stationary probability of a table
 *      entry.  These calls count, for the two-pass coder at k = 0 (-cp 2, file _0 of ref / sig / sign), every decision
 *      the coder would code in the given data: counts[entry][symbol], entry = the table index the coder reads (the raw
 *      index clamped to the table, so bit-plane 15 of a group counts where the coder looks: in the next group when
 *      n_bitplanes = 15).  At k = 0 the decisions depend on the coefficients alone, never on a table: a context needs
 *      none set.  All-zero codeblocks contribute nothing; a codeblock with MSB > 15 contributes nothing and raises
 *      picsong_range_flag.  The counts are exact integers, identical from run to run.
 *      picsong_train_begin: allocates and zeroes uint64[n_ref + n_sig + n_sign][2] for the three component slots.
 *        `geometry`: n_bitplanes, n_subbands and the three context counts; n_ref / n_sig / n_sign of 0 are derived for
 *        the context's wl (IO/IOManager.ipp:431-433).  A second begin starts over.  picsong_train_info returns the
 *        geometry with its section sizes filled in (n_files 3, n_bp_files 1, n_tables 1, cp 2): what
 *        picsong_lut_from_counts, picsong_lut_save and picsong_ctx_set_lut take.
 *      picsong_train_coeffs: the stage-level seam; d_coeffs as picsong_bpc_encode takes it (Mallat T[AW*AH]).
 *      picsong_train_frames: n = 1..64 padded u8 frames, frame f at d_frames + f * frame_stride bytes, through the
 *        forward transform of the encode calls (level shift; 9/7 with the context's qs) and ONE statistics launch over
 *        the n x nCB codeblocks; into slot 0.  16-byte aligned frames take the vector kernels and the 16-bit coefficient
 *        form as picsong_encode_frames does; any other pointer or stride is accepted too (per-column kernels, 32-bit
 *        arrays, a transform launch a frame): same counts, slower.
 *      picsong_train_rgb_frame: RCT / ICT + transform as picsong_encode_rgb_frame; component c into slot c.
 *      picsong_train_rgb_frames (declared with the n-frame RGB search calls below): n = 1..21 frames as
 *        picsong_encode_rgb_frames addresses them, one transform and a statistics launch a component; the same counts.
 *      picsong_train_counts: synchronises `stream` and copies slot `component` to h_counts ([entry][2]: zeros, ones;
 *        capacity_entries >= the entry count); with h_counts == NULL it returns the entry count instead.
 *      All but picsong_train_counts are asynchronous on `stream` and accumulate across calls; picsong_train_reset
 *      zeroes the three slots, picsong_train_end frees them.
 *      Refused (PICSONG_ERR_ARG, nothing launched): training calls before picsong_train_begin; -cp 3 and -k > 0
 *      contexts (they code other decisions: the bit-plane files _1.._14 and the cp_sig / cp_sign sections are not
 *      trained); a geometry with n_bitplanes < 1, n_subbands < 1 or a context count < 1, or with more entries than a
 *      workgroup's on-chip copy holds (4864; wl = 7 at 15 / 3 / 1 / 4 / 9 has 4620); the n / stride / null checks of the
 *      encode calls; picsong_train_rgb_frame on a grey context and picsong_train_frames on an RGB one. ---- */
int picsong_train_begin(picsong_ctx *ctx, const picsong_lut_info *geometry);
int picsong_train_info(const picsong_ctx *ctx, picsong_lut_info *info);
int picsong_train_reset(picsong_ctx *ctx);
int picsong_train_end(picsong_ctx *ctx);
int picsong_train_coeffs(picsong_ctx *ctx, int component, const void *d_coeffs, void *stream);
int picsong_train_frames(picsong_ctx *ctx, int n, const uint8_t *d_frames, size_t frame_stride, void *stream);
int picsong_train_rgb_frame(picsong_ctx *ctx, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b, void *stream);
int picsong_train_counts(picsong_ctx *ctx, int component, void *stream, uint64_t *h_counts, size_t capacity_entries);
/* Host only.  picsong_lut_from_counts: the table of the counts.  For every entry with t = zeros + ones > 0:
 *   p = clamp((zeros * 2^precision + t / 2) / t, 1, 2^precision - 1) in 64-bit integer arithmetic -- the probability of
 *   a 0 in the coder's fixed point, rounded to nearest, kept off the two values that end a codeword at once; an entry
 *   with t = 0 keeps prior_table's value, or 2^(precision - 1) without a prior (the 64 of the shipped files and of the
 *   loader's group fill).  info: complete (picsong_train_info / picsong_lut_load); counts: [entry][2]; table and
 *   prior_table: n_ref + n_sig + n_sign ints.
 * picsong_lut_save: writes header.txt (LUT_N_FILES;3, AMOUNT_OF_BITPLANE_FILES;1) and {ref,sig,sign}{,R,G,B}.txt_0
 *   (component 0 = un-suffixed, 1/2/3 = R/G/B as picsong_lut_load) in the reference's text format, every group
 *   (level 0..wl-1 x subband 0..n_subbands-1, then (wl, 0): LL) with all its n_bitplanes planes, so that
 *   picsong_lut_load(folder, component, wl, fill, ..) returns exactly `table` for any fill.  Creates `folder` (one
 *   level) if absent; PICSONG_ERR_IO if it cannot be created or written; writes only those files inside it.  The
 *   section sizes of `info` must be the ones wl implies.
 *   A TRAINED FOLDER BELONGS TO THE wl IT WAS WRITTEN FOR: the loader reads group (wl, 0) as LL, so at another wl the
 *   LL statistics land on a detail subband's group (the shipped folders are laid out for wl = 5 in the same way). */
int picsong_lut_from_counts(const picsong_lut_info *info, const uint64_t *counts, const int32_t *prior_table, int32_t *table);
int picsong_lut_save(const char *folder, int component, const picsong_lut_info *info, int wl, const int32_t *table);

/* ---- encode to a target size (JPEG 2000 style rate control, OpenJPEG -r / Kakadu -rate; the reference has no
 *      counterpart): the 9/7 calls above with the quantiser gain qs CHOSEN so that the codestream meets a size.
 *      The grid.  The header stores qs as (int)(qs * 10000) in 14 bits and a decoder reads q(j) = (float)(j / 10000.0):
 *      only the values q(j), j = 1..16383, ever reach a decoder, and for 1143 of them the float product stores j - 1
 *      (7, 14, 28, ... 16383).  The search runs over the header-exact grid G, the 15240 values of j the header carries
 *      unchanged (1 2 3 4 5 6 8 9 ... 16382).  picsong_rate_qs (host only): q(j); PICSONG_ERR_ARG for j outside 1..16383
 *      or not in G.
 *      The result.  Size against j is not monotone (a finer quantiser can code a few shorts shorter), so the result is
 *      defined by a procedure, not as a maximum: with G' = the entries of G inside [j_min, j_max] (j_min = j_max = 0: all
 *      of G; else 1 <= j_min <= j_max <= 16383; a range without a grid entry is PICSONG_ERR_ARG),
 *          lo = -1, hi = len(G');  while hi - lo > 1: mid = (lo + hi) / 2;  size(G'[mid]) <= target ? lo = mid : hi = mid
 *      and the result is G'[lo]; size(j) = the codestream length in shorts, header and terminator included, as
 *      picsong_last_total reports it, summed over the call's frames / components.  14 probes over the whole grid.
 *      On success *h_j is the result, the streams are BYTE-IDENTICAL to what picsong_encode_frame / picsong_encode_frames /
 *      picsong_encode_rgb_frame write on a context created with qs = q(*h_j) (the header carries that qs), and
 *      h_total(s) receive their lengths (1, n and 3 of them).  When nothing fits (size(G'[0]) > target) the call returns
 *      PICSONG_ERR_RATE with *h_j = 0; the streams are then unspecified, and no short beyond picsong_max_stream_shorts
 *      per stream is ever written.
 *      How.  The transform runs once with unit steps into float arrays; each round of the search quantises them for up
 *      to three candidates (the midpoint and the two midpoints that follow from either outcome: two steps of the
 *      procedure) and codes them in one batched coder launch; only the result is packed.  The calls are SYNCHRONOUS on
 *      `stream`: one read-back of the candidates' lengths per round, through pinned memory, and one at the end.  The
 *      lengths come back through h_total(s), and stay where the plain calls leave theirs (picsong_last_total after the
 *      single-frame call, picsong_last_totals / picsong_copy_last_totals after all three).
 *      The context's own qs is NOT changed.  picsong_ctx_set_qs sets it -- re-deriving everything picsong_ctx_create
 *      derives from qs, tables and buffers kept -- so that a caller codes the rest of a video at the chosen qs without a
 *      new context; it refuses qs <= 0 and qs > q(16383) = 1.6383, what the header cannot store.  (picsong_ctx_create
 *      keeps the reference launcher's range (0, 1]; the grid is the header's whole range, so a result above j = 10000 --
 *      an easy image and a generous target -- is reached through picsong_ctx_set_qs, by a decoder too: create the context
 *      at qs = 1 and set the header's value.)
 *      picsong_range_flag accumulates over every probe of a call: a probe FINER than the result can raise it even when
 *      the result's own stream would not.
 *      The context grows its workspace at the first call: one float array per frame and the batch buffers of 3 n frames.
 *      picsong_encode_frames_rate: n = 1..16 (the candidates share the 64-frame batched grid), target_shorts for the SUM of
 *      the n streams, strides and alignment as picsong_encode_frames; any -k.  picsong_encode_rgb_frame_rate:
 *      target_shorts for the sum of the three components' streams; one candidate a round (the coder maps a launch's frames
 *      to the component tables for three frames only); same result.
 *      Refused (PICSONG_ERR_ARG, nothing launched): lossless contexts, -cp 3 contexts, the grey calls on an RGB context and
 *      the RGB call on a grey one, target_shorts = 0, a bad range, and the null / stride / alignment checks of the plain
 *      calls (h_j and h_total(s) must not be null). ---- */
int picsong_rate_qs(int j, float *qs);
int picsong_ctx_set_qs(picsong_ctx *ctx, float qs);
int picsong_encode_frame_rate(picsong_ctx *ctx, const uint8_t *d_frame, int iter, size_t target_shorts, int j_min, int j_max,
                              uint16_t *d_stream, void *stream, int *h_j, int *h_total);
int picsong_encode_frames_rate(picsong_ctx *ctx, int n, const uint8_t *d_frames, size_t frame_stride, int first_iter,
                               size_t target_shorts, int j_min, int j_max, uint16_t *d_streams, size_t stream_stride,
                               void *stream, int *h_j, int *h_totals);
int picsong_encode_rgb_frame_rate(picsong_ctx *ctx, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b, int header_mask,
                                  size_t target_shorts, int j_min, int j_max, uint16_t *d_streams, size_t stream_stride,
                                  void *stream, int *h_j, int *h_totals);

/* ---- encode to a target quality (OpenJPEG -q / Kakadu's quality targets; the reference has no counterpart): the 9/7
 *      calls with the quantiser gain qs CHOSEN so that the decoded frames stay within a distortion limit.
 *      The measure is the SSE, the sum of squared differences over the VISIBLE W x H samples (padding is not counted),
 *      an exact integer.  picsong_psnr_to_sse / picsong_sse_to_psnr (host only) convert for 8-bit samples:
 *      max_sse = floor(65025 * samples / 10^(dB / 10)) in double arithmetic, PSNR = 10 log10(65025 * samples / sse), HUGE_VAL
 *      for sse = 0; PICSONG_ERR_ARG for null pointers, samples = 0 and a PSNR that is not finite.
 *      picsong_frames_sse measures: d_sse[f] = the SSE of frame f of d_a against frame f of d_b, n = 1..64 padded frames
 *      (row stride AW) a_stride / b_stride bytes apart; d_sse is a device uint64[n], overwritten.  ASYNCHRONOUS on
 *      `stream`, any pointer alignment (16-byte aligned pointers and strides take the vector loads, same result), any
 *      context -- lossless, -cp 3, grey or RGB: only its geometry is used; an RGB frame is three planes, n = 3.  Refused
 *      (PICSONG_ERR_ARG, nothing launched): null pointers, n outside 1..64, a stride below a padded frame when n > 1.
 *      The search runs over the grid G and the sub-ranges of the rate calls above.  SSE against j is not monotone either
 *      (a finer quantiser can decode a few squares worse), so the result is again a procedure's, the mirror of the rate
 *      one: with G' = the entries of G inside [j_min, j_max],
 *          lo = -1, hi = len(G');  while hi - lo > 1: mid = (lo + hi) / 2;  sse(G'[mid]) <= max_sse ? hi = mid : lo = mid
 *      and the result is G'[hi], the coarsest quantiser the bisection finds that meets the limit; sse(j) = the SSE between
 *      the input and what picsong_decode_frame / picsong_decode_rgb_frame return for the stream coded at q(j), summed
 *      over the call's frames / the three planes.  13 or 14 probes over the whole grid.  max_sse = 0 is a legal request.
 *      On success *h_j is the result, the streams are BYTE-IDENTICAL to the plain encode calls' on a context at q(*h_j)
 *      (the header carries that qs), h_total(s) receive their lengths and h_sse the SSE per frame / per plane R, G, B
 *      (1, n and 3 of each).  When nothing meets the limit (hi = len(G')) the call returns PICSONG_ERR_QUALITY with
 *      *h_j = 0; the streams are then unspecified, and no short beyond picsong_max_stream_shorts per stream is written.
 *      How.  The coder is lossless over the quantised coefficients, so a probe needs no coder launch: the transform runs
 *      once with unit steps; per candidate the quantise pass writes int32 coefficients, the synthesis at q(j) -- the
 *      dividing kernels, whose pixels every reciprocal form is verified against -- writes clamped pixels, and the SSE
 *      kernel compares them with the input.  Up to three candidates a round (two steps of the procedure), back to back
 *      over one set of n-frame buffers; one read-back through pinned memory per round.  The result is then quantised,
 *      coded and packed as the rate calls' final step.  The calls are SYNCHRONOUS on `stream`.  The lengths stay where the
 *      plain calls leave theirs.  The context's own qs is NOT changed (picsong_ctx_set_qs).  picsong_range_flag sees only
 *      the result's own encode.  n = 1..16; strides and alignment as the matching rate call; any -k.
 *      Refused (PICSONG_ERR_ARG, nothing launched, outputs untouched): lossless and -cp 3 contexts, the grey calls on an
 *      RGB context and the RGB call on a grey one, a bad range or one without a grid entry, the null / stride / alignment
 *      checks of the matching rate call (h_j, h_total(s) and h_sse must not be null), a context without its table. ---- */
int picsong_psnr_to_sse(double psnr_db, uint64_t samples, uint64_t *max_sse);
int picsong_sse_to_psnr(uint64_t sse, uint64_t samples, double *psnr_db);
int picsong_frames_sse(picsong_ctx *ctx, int n, const uint8_t *d_a, size_t a_stride, const uint8_t *d_b, size_t b_stride,
                       uint64_t *d_sse, void *stream);
int picsong_encode_frame_quality(picsong_ctx *ctx, const uint8_t *d_frame, int iter, uint64_t max_sse, int j_min, int j_max,
                                 uint16_t *d_stream, void *stream, int *h_j, int *h_total, uint64_t *h_sse);
int picsong_encode_frames_quality(picsong_ctx *ctx, int n, const uint8_t *d_frames, size_t frame_stride, int first_iter,
                                  uint64_t max_sse, int j_min, int j_max, uint16_t *d_streams, size_t stream_stride,
                                  void *stream, int *h_j, int *h_totals, uint64_t *h_sse);
int picsong_encode_rgb_frame_quality(picsong_ctx *ctx, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b, int header_mask,
                                     uint64_t max_sse, int j_min, int j_max, uint16_t *d_streams, size_t stream_stride,
                                     void *stream, int *h_j, int *h_totals, uint64_t *h_sse);

/* ---- the search over n RGB frames: a colour video has ONE header, so one qs for all its frames; these calls choose
 *      it over the first n of them instead of over frame 0 alone.  The semantics are those of the two sections above,
 *      unchanged -- the grid G, the sub-range G', the two bisection procedures that define the result -- with
 *      size(j) = the sum of the 3 n stream lengths and sse(j) = the sum over the 3 n planes; target_shorts / max_sse apply
 *      to those sums.  n = 1..21.  Addressing, first_iter, header_mask and the placement of the streams are
 *      picsong_encode_rgb_frames': frame f's planes frame_stride bytes after d_r / d_g / d_b, its component c's stream at
 *      d_streams + (3 f + c) * stream_stride, the populated header on the components of header_mask of the frame with
 *      first_iter + f == 0.
 *      On success *h_j is the result, the 3 n streams are BYTE-IDENTICAL to picsong_encode_rgb_frames' on a context at
 *      q(*h_j) with the same first_iter and header_mask (the header carries that qs), h_totals[3 n] their lengths and
 *      h_sse[3 n] the SSE per plane (frame f's R, G, B at 3 f ..); the lengths also stay where the plain call leaves
 *      them (picsong_last_totals(3 n) / picsong_copy_last_totals).  Nothing fits: PICSONG_ERR_RATE / PICSONG_ERR_QUALITY
 *      with *h_j = 0; no short beyond picsong_max_stream_shorts per stream is ever written.  SYNCHRONOUS on `stream`; the
 *      context's own qs is NOT changed; any -k.
 *      How.  A size round codes three candidates in one batched coder launch where 3 * 3 n <= 64 planes (n <= 7: plane
 *      c * 3 n + 3 f + comp still meets table comp), else one.  A quality round measures three candidates back to back
 *      over one set of 3 n-plane buffers; a probe is the quantise pass, ONE synthesis over the 3 n planes and ONE kernel
 *      that applies the inverse ICT to the float planes and sums the squared error against the input without writing a
 *      pixel (PICSONG_RGB_SSE_FUSED=0, read per call, keeps the separate colour transform and three SSE launches a frame:
 *      same sums).  PICSONG_RATE_K=1 keeps one candidate a round.  The result is the procedure's whatever the number of
 *      candidates.  picsong_range_flag ACCUMULATES OVER EVERY PROBE MADE by a size search -- with three candidates a
 *      round that includes probes the procedure ignores, and probes finer than the result -- so it can be raised where
 *      the result's own stream would not raise it; a quality search's probes run no coder and it sees the result's own
 *      encode only.  The single-frame calls above keep one candidate a size round, and their results, range flag included.
 *      picsong_train_rgb_frames (see the training section): n = 1..21 frames through one transform and three statistics
 *      launches, component c of every frame into slot c; the counts of n picsong_train_rgb_frame calls.
 *      Refused (PICSONG_ERR_ARG, nothing launched, outputs untouched): everything picsong_encode_rgb_frames refuses
 *      (null pointers, a grey or -cp 3 context, n outside 1..21, a stream stride below the worst case, with n > 1 a
 *      frame_stride below a padded plane or one that makes frames overlap, tables that differ in geometry); everything
 *      the single-frame search calls refuse (lossless contexts, target_shorts = 0, a bad range or one without a grid
 *      entry, null h_j / h_totals / h_sse, a context without its tables); planes that are not 4-byte aligned; with
 *      n > 1 a frame_stride that is not a multiple of 4. ---- */
int picsong_encode_rgb_frames_rate(picsong_ctx *ctx, int n, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b,
                                   size_t frame_stride, int first_iter, int header_mask, size_t target_shorts, int j_min,
                                   int j_max, uint16_t *d_streams, size_t stream_stride, void *stream, int *h_j, int *h_totals);
int picsong_encode_rgb_frames_quality(picsong_ctx *ctx, int n, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b,
                                      size_t frame_stride, int first_iter, int header_mask, uint64_t max_sse, int j_min,
                                      int j_max, uint16_t *d_streams, size_t stream_stride, void *stream, int *h_j,
                                      int *h_totals, uint64_t *h_sse);
int picsong_train_rgb_frames(picsong_ctx *ctx, int n, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b,
                             size_t frame_stride, void *stream);

/* ---- encode to a target SSIM (x264 --ssim / ffmpeg's ssim filter measure it; the reference has no counterpart): the
 *      quality calls above with a structural measure for the SSE.  The measure is x264's integer 8 x 8 SSIM of 8-bit
 *      samples over the VISIBLE W x H part, W, H >= 8: windows of 8 x 8 samples at the origins (4 x, 4 y),
 *      x < nx = (W - 8) / 4 + 1, y < ny = (H - 8) / 4 + 1 (columns from 4 (nx + 1) and rows from 4 (ny + 1) on belong to
 *      no window); per window the exact sums s1 = sum a, s2 = sum b, ss = sum a^2 + sum b^2, s12 = sum a b and, with
 *      c1 = 416, c2 = 235963,
 *          A = 2 s1 s2 + c1, B = 2 (64 s12 - s1 s2) + c2, C = s1^2 + s2^2 + c1, E = 64 ss - s1^2 - s2^2 + c2,
 *          v = ((double)A * (double)B) / ((double)C * (double)E),  q = (int64)floor(v * 2^24)   (q <= 2^24, may be negative).
 *      The DSSIM sum of a pair of planes is windows * 2^24 - sum q: an exact, order-independent, non-negative integer,
 *      0 for equal planes; SSIM = 1 - dssim / (windows * 2^24).  Host-only helpers: picsong_ssim_windows gives nx * ny
 *      (PICSONG_ERR_ARG below 8 x 8); picsong_ssim_to_dssim gives floor(((1 - ssim) * windows) * 2^24) in double
 *      arithmetic in that order, ssim in [-1, 1], windows > 0 (for a limit over several planes pass the windows of all
 *      of them); picsong_dssim_to_ssim the way back.
 *      picsong_frames_dssim measures: d_dssim[f] = the DSSIM sum of frame f of d_a against frame f of d_b; n, strides,
 *      alignment (any: 4-byte aligned pointers and strides take dword loads), asynchrony and refusals as
 *      picsong_frames_sse, and PICSONG_ERR_ARG on a context below 8 x 8.  d_dssim is a device uint64[n], overwritten.
 *      The search calls are picsong_encode_frame_quality / picsong_encode_frames_quality /
 *      picsong_encode_rgb_frames_quality with dssim(j) for sse(j): the same grid, sub-range and bisection
 *          lo = -1, hi = len(G');  while hi - lo > 1: mid = (lo + hi) / 2;  dssim(G'[mid]) <= max_dssim ? hi = mid : lo = mid
 *      result G'[hi]; dssim(j) = the DSSIM sum of the input against what picsong_decode_frame / picsong_decode_rgb_frame
 *      return for the stream coded at q(j), summed over the call's frames (RGB: over the R, G and B planes of every
 *      frame).  h_dssim receives 1, n or 3 n per-plane values; PICSONG_ERR_QUALITY with *h_j = 0 when nothing in the
 *      range meets the limit; the streams are the plain encode calls' at q(*h_j) byte for byte; n = 1..16 grey, 1..21
 *      RGB (a single RGB frame is n = 1); strides, alignment rules, synchrony and refusals as the quality calls', and
 *      PICSONG_ERR_ARG on a context below 8 x 8.  Three candidates a round (PICSONG_RATE_K=1: one), one read-back a
 *      round; a probe runs no coder: quantise, dividing synthesis, ssim_kernel (RGB: the inverse ICT writes the pixels
 *      first). ---- */
int picsong_ssim_windows(int w, int h, uint64_t *windows);
int picsong_ssim_to_dssim(double ssim, uint64_t windows, uint64_t *max_dssim);
int picsong_dssim_to_ssim(uint64_t dssim, uint64_t windows, double *ssim);
int picsong_frames_dssim(picsong_ctx *ctx, int n, const uint8_t *d_a, size_t a_stride, const uint8_t *d_b, size_t b_stride,
                         uint64_t *d_dssim, void *stream);
int picsong_encode_frame_ssim(picsong_ctx *ctx, const uint8_t *d_frame, int iter, uint64_t max_dssim, int j_min, int j_max,
                              uint16_t *d_stream, void *stream, int *h_j, int *h_total, uint64_t *h_dssim);
int picsong_encode_frames_ssim(picsong_ctx *ctx, int n, const uint8_t *d_frames, size_t frame_stride, int first_iter,
                               uint64_t max_dssim, int j_min, int j_max, uint16_t *d_streams, size_t stream_stride,
                               void *stream, int *h_j, int *h_totals, uint64_t *h_dssim);
int picsong_encode_rgb_frames_ssim(picsong_ctx *ctx, int n, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b,
                                   size_t frame_stride, int first_iter, int header_mask, uint64_t max_dssim, int j_min,
                                   int j_max, uint16_t *d_streams, size_t stream_stride, void *stream, int *h_j,
                                   int *h_totals, uint64_t *h_dssim);

/* ---- frames as applications hold them (the reference reads files only, IO/IOManager.ipp:72-112; nvJPEG2000 and
 *      friends take a pitched image descriptor): W x H pixels (the context's unpadded -xSize / -ySize) at a byte pitch,
 *      one byte a pixel or interleaved RGB(A), converted ON THE DEVICE to and from the padded planar u8 planes every
 *      other call takes -- no host pad, no caller-written kernels.
 *      picsong_image: `data` is the DEVICE address of the first pixel, row y at data + y * pitch (pitch >= W * bpp, any
 *      value: rows need not be packed).  PLANAR3: the R, G, B planes plane_stride bytes apart (plane_stride is ignored
 *      by the other layouts).  Frame f of a call at data + f * frame_stride.
 *      The padded side: `planes` planes of P = AW * AH bytes back to back per frame (1 for GREY8, 3 -- R, G, B -- for
 *      every other layout), row stride AW, frames padded_stride bytes apart.
 *      picsong_ingest_frames pads with the mirror rule of picsong_pad_frame_host (column W + j = column W - 1 - j,
 *      padded row H + r = padded row H - 1 - r) and de-interleaves in the same pass; the alpha byte is ignored.  It
 *      reads no byte outside [y * pitch, y * pitch + W * bpp) of rows 0 .. H - 1.  picsong_emit_frames crops and
 *      interleaves; alpha is written as 255; it writes no byte outside those ranges (not the pitch gap, not past the last
 *      row).  Both are ASYNCHRONOUS on `stream`, take any context (only its geometry is used) and n = 1..64 frames.
 *      Alignment: none required.  An image side whose pointer, pitch and strides are 4-byte aligned with a padded side
 *      whose pointer and stride are 16-byte aligned takes the vector kernels (dword / dwordx4 accesses; an RGB24 group of
 *      four pixels is three dwords repacked with byte permutes); anything else the per-byte kernels: same bytes, slower.
 *      After an ingest every existing call composes unchanged on the padded planes: picsong_encode_frame(s), the rate,
 *      quality and training calls, the stripes; an emit takes what any decode call wrote at full size.
 *      Whole-frame calls: ingest into a 16-byte aligned buffer the context grows (so the vector kernels run whenever
 *      the image side allows), then the plain frame sequence -- and the mirror for decoding.
 *        picsong_encode_images (grey contexts, n = 1..64): byte-identical to picsong_encode_frames on host-padded frames.
 *        picsong_encode_rgb_image (RGB contexts, one frame): byte-identical to picsong_encode_rgb_frame.
 *        picsong_decode_images / picsong_decode_rgb_image: the W x H crop of picsong_decode_frames' /
 *        picsong_decode_rgb_frame's output, in the layout of `dst`.
 *      Lengths are reported where the plain calls leave them (picsong_last_totals / picsong_copy_last_totals); -cp 3 is
 *      accepted wherever the underlying plain call accepts it (none of these four does).
 *      Refused (PICSONG_ERR_ARG, nothing launched, outputs untouched): null pointers; an unknown layout; pitch < W * bpp;
 *      plane_stride (PLANAR3) below (H - 1) * pitch + W; with n > 1 a frame_stride below the bytes a frame spans or a
 *      padded_stride below planes * P; n outside 1..64; AW - W > W or AH - H > H (the rule picsong_pad_frame_host
 *      refuses); in the whole-frame calls also a colour layout on a grey context, GREY8 on an RGB one, and what the
 *      plain call refuses (stream strides, -cp 3). ---- */
#define PICSONG_LAYOUT_GREY8   0   /* 1 byte a pixel; grey contexts */
#define PICSONG_LAYOUT_PLANAR3 1   /* R, G, B planes plane_stride bytes apart, each at `pitch` */
#define PICSONG_LAYOUT_RGB24   2
#define PICSONG_LAYOUT_BGR24   3
#define PICSONG_LAYOUT_RGBA32  4   /* A ignored on input, 255 on output */
#define PICSONG_LAYOUT_BGRA32  5
#define PICSONG_LAYOUT_GREY16  6   /* 2 bytes a pixel, little-endian; deep contexts */
#define PICSONG_LAYOUT_PLANAR3_16 7 /* deep RGB contexts: three uint16 planes plane_stride bytes apart */
#define PICSONG_LAYOUT_RGB48   8   /* ... interleaved R, G, B, 6 bytes a pixel */
#define PICSONG_LAYOUT_RGBA64  9   /* ... interleaved R, G, B, A, 8 bytes; A ignored on input, 2^bd - 1 on output */
typedef struct picsong_image { void *data; size_t pitch; size_t plane_stride; int layout; } picsong_image;
int picsong_ingest_frames(picsong_ctx *ctx, int n, const picsong_image *src, size_t frame_stride, uint8_t *d_padded,
                          size_t padded_stride, void *stream);
int picsong_emit_frames(picsong_ctx *ctx, int n, const uint8_t *d_padded, size_t padded_stride, const picsong_image *dst,
                        size_t frame_stride, void *stream);
int picsong_encode_images(picsong_ctx *ctx, int n, const picsong_image *src, size_t frame_stride, int first_iter,
                          uint16_t *d_streams, size_t stream_stride, void *stream);
int picsong_decode_images(picsong_ctx *ctx, int n, const uint16_t *d_streams, size_t stream_stride, const picsong_image *dst,
                          size_t frame_stride, void *stream);
int picsong_encode_rgb_image(picsong_ctx *ctx, const picsong_image *src, int header_mask, uint16_t *d_streams,
                             size_t stream_stride, void *stream);
int picsong_decode_rgb_image(picsong_ctx *ctx, const uint16_t *d_streams, size_t stream_stride, const picsong_image *dst,
                             void *stream);

/* ---- deep contexts: 9- to 16-bit grey samples (cinema, broadcast, medical, remote sensing).  A context created with
 *      bit_depth 9..16 (components 1, is_rgb 0; an RGB one: "deep RGB contexts" below) takes its frames as native (little-endian)
 *      uint16_t samples v in [0, 2^bd - 1]; off = 2^(bd-1).  Only the transform's two ends differ from an 8-bit context:
 *        forward   5/3: x = (int32)v - off;  9/7: x = (float)v - (float)off (offsetImage with the depth as a parameter).
 *                  v is read UNSIGNED (65535 is never -1); a v above 2^bd - 1 is the caller's error: coded as it is,
 *                  decoded clamped.
 *        inverse   5/3: clamp(x + off, 0, 2^bd - 1);  9/7: clamp(rintf((x + off) + 0.01f), 0, 2^bd - 1), NaN -> 0: the
 *                  8-bit arithmetic with 255 replaced by 2^bd - 1 (the reference hard-codes 255: this is the extension).
 *        padding   the mirror rule of picsong_pad_frame_host on 2-byte samples (picsong_pad_frame16_host).
 *        header    both depth fields carry bd; nothing else changes: a deep stream has the 8-bit stream's layout.
 *      Between the ends a deep context ALWAYS has the 32-bit coefficient form, one launch a level, no fused head or
 *      tail (the int16 form where the bound allows it, and fused deep ends, are follow-ups: DESIGN.md 4.17).
 *      Range: the coders code magnitudes below 2^15.  picsong_depth_range_guaranteed (host only, no context) says
 *      whether EVERY frame of that depth stays below: *yes = the bound the 16-bit coefficient form uses, with
 *      max|sample| = 2^(bd-1) -- for 5/3 that is bd <= 12 (2048 x 2.8601^2 + 64 < 30000); for 9/7 it depends on qs and
 *      wl.  Where it says no, the calls do not refuse: a frame whose coefficients reach 2^15 raises picsong_range_flag,
 *      exactly as an out-of-range array through picsong_bpc_encode does (full-range 16-bit noise through 5/3 reaches
 *      |c| ~ 10^5; smooth 14-bit content stays below 10^4).
 *      Work unchanged on a deep context (they take T arrays): picsong_dwt_forward, picsong_dwt_inverse,
 *      picsong_bpc_encode / _decode (_component), picsong_bitstream_pack / _unpack, picsong_train_coeffs,
 *      picsong_last_total(s), picsong_copy_last_totals, picsong_range_flag; picsong_level_shift_inv clamps to 2^bd - 1
 *      there; picsong_ctx_set_decode_drop stays allowed (its effect is the coder's).
 *      Refused on a deep context (PICSONG_ERR_ARG, nothing launched, outputs untouched): every call that takes or
 *      returns uint8_t frames -- picsong_encode_frame(s), picsong_decode_frame(s) and their _reduced / _window forms,
 *      the stripe and band calls on frames, picsong_train_frames, the rate and quality calls, picsong_frames_sse,
 *      picsong_level_shift_fwd, picsong_dwt_forward_u8, picsong_rgb_forward / _inverse -- and the 8-bit layouts in the
 *      layout and image calls.  Refused on an 8-bit context: the three *16 device calls below and GREY16.
 *      picsong_level_shift_fwd16: the level shift alone, uint16[P] -> T[P] (2-byte aligned d_in).
 *      picsong_dwt_forward_u16: the mirror of picsong_dwt_forward_u8 -- level shift in level 0's load stage.
 *      picsong_encode_frames16 / picsong_decode_frames16: n = 1..64 frames, ONE launch per stage (grid.z = frame).
 *        Frame f is a padded uint16[AW*AH] at (char *)d_frames + f * frame_stride; frame_stride in BYTES, even,
 *        >= 2 P, ignored for n = 1.  Streams, headers (first_iter), lengths and -cp 2 with any -k as
 *        picsong_encode_frames / picsong_decode_frames; -cp 3 is refused.  Pointers need 2-byte alignment.  16-byte
 *        aligned pointers and strides take the vector kernels (one 8-byte load / store of a lane's four samples);
 *        anything else the per-column kernels (encode) or a separate clamp pass (decode): the same bytes.  Decoding
 *        writes exactly the 2 P bytes of each frame.  PICSONG_DEEP_NOFUSE=1 (read per call) takes the element-wise
 *        level shift / clamp passes beside the T-input level 0 / T-output finest level instead: the same bytes.
 *      GREY16 in picsong_ingest_frames / picsong_emit_frames: the padded side is uint16 planes, passed through the
 *        uint8_t * parameter, padded_stride in bytes (>= 2 P); pitch >= 2 W; data, pitch and the strides need 2-byte
 *        alignment (refused otherwise); no byte outside [y * pitch, y * pitch + 2 W) of rows 0 .. H - 1 is read or
 *        written.  picsong_encode_images / picsong_decode_images accept GREY16 on deep contexts, byte-identical to the
 *        *16 frame calls on host-padded frames. ---- */
int picsong_depth_range_guaranteed(int bit_depth, int lossy, int wl, float qs, int *yes);              /* host only */
int picsong_pad_frame16_host(const uint16_t *in, int w, int h, uint16_t *out, int aw, int ah);         /* host only */
int picsong_level_shift_fwd16(picsong_ctx *ctx, const uint16_t *d_in, void *d_out, void *stream);
int picsong_dwt_forward_u16(picsong_ctx *ctx, const uint16_t *d_in, void *d_out, void *stream);
int picsong_encode_frames16(picsong_ctx *ctx, int n, const uint16_t *d_frames, size_t frame_stride, int first_iter,
                            uint16_t *d_streams, size_t stream_stride, void *stream);
int picsong_decode_frames16(picsong_ctx *ctx, int n, const uint16_t *d_streams, size_t stream_stride,
                            uint16_t *d_frames_out, size_t frame_stride, void *stream);

/* ---- batched RGB frames: n = 1..21 colour frames through ONE launch per stage (3 n <= 64, the batched grid's limit).
 *      Every stage launches once over 3 n planes: plane z is component z % 3 of frame z / 3, component c codes with
 *      table c.  Every stream is byte-identical to what picsong_encode_rgb_frame writes for that frame, every decoded
 *      plane to picsong_decode_rgb_frame's.
 *      Addressing: d_r / d_g / d_b are frame 0's padded u8[AW*AH] planes, frame f's lie f * frame_stride bytes after
 *      each of them -- three separate arrays (frame_stride >= P) and R, G, B back to back per frame (frame_stride = 3 P)
 *      alike; frame_stride is ignored for n = 1.  The stream of frame f, component c lands at (is read from)
 *      d_streams + (3 f + c) * stream_stride shorts, stream_stride >= picsong_max_stream_shorts.
 *      Headers: header_mask (bits 0..2) names the components that carry the populated header on the frame with
 *      first_iter + f == 0; every other frame carries none (a video: mask 7; an image: mask 1).
 *      Lengths: the 3 n of them through picsong_last_totals(ctx, stream, 3 n, ..) / picsong_copy_last_totals.
 *      Alignment: as the single-frame call -- the fused head runs when all three planes are 16-byte aligned and
 *      frame_stride is a multiple of 16, else the separate colour-transform kernel (one launch a frame: same streams,
 *      slower); decoding, planes and frame_stride 4-byte aligned take the fused tails (grid.z = frame), anything else the
 *      separate inverse colour transform (one launch a frame).
 *      -cp 2 RGB contexts, any -k, both coefficient forms, 5/3 and 9/7.
 *      picsong_encode_rgb_images / picsong_decode_rgb_images: n frames in a colour layout of picsong_image, frame f at
 *      data + f * frame_stride -- ONE ingest (emit) into (from) the context's aligned buffer, 3 planes a frame, then the
 *      calls above.
 *      Refused (PICSONG_ERR_ARG, nothing launched, outputs untouched): null pointers; a grey context; -cp 3; n outside
 *      1..21; with n > 1 a frame_stride below a padded plane or one that makes a frame's planes overlap the next
 *      frame's; a stream stride below a worst-case stream; component tables of different geometry; the image calls also
 *      everything the layout calls refuse, and GREY8. ---- */
int picsong_encode_rgb_frames(picsong_ctx *ctx, int n, const uint8_t *d_r, const uint8_t *d_g, const uint8_t *d_b,
                              size_t frame_stride, int first_iter, int header_mask,
                              uint16_t *d_streams, size_t stream_stride, void *stream);
int picsong_decode_rgb_frames(picsong_ctx *ctx, int n, const uint16_t *d_streams, size_t stream_stride,
                              uint8_t *d_r, uint8_t *d_g, uint8_t *d_b, size_t frame_stride, void *stream);
int picsong_encode_rgb_images(picsong_ctx *ctx, int n, const picsong_image *src, size_t frame_stride, int first_iter,
                              int header_mask, uint16_t *d_streams, size_t stream_stride, void *stream);
int picsong_decode_rgb_images(picsong_ctx *ctx, int n, const uint16_t *d_streams, size_t stream_stride,
                              const picsong_image *dst, size_t frame_stride, void *stream);

/* ---- deep RGB contexts: 9- to 16-bit colour samples (HDR and broadcast video, cinema masters, camera and scanner RGB).
 *      A context created with bit_depth 9..16, components 3 and is_rgb 1 takes a frame as three padded planes of native
 *      (little-endian) uint16_t samples v in [0, 2^bd - 1], padded by the rule of picsong_pad_frame16_host;
 *      off = 2^(bd-1), mx = 2^bd - 1.  The colour transforms are the 8-bit ones on level-shifted 16-bit samples:
 *        forward 5/3 (RCT)  R' = (int32)R - off (likewise G', B'); c0 = (R' + 2 G' + B') >> 2, c1 = B' - G', c2 = R' - G'.
 *        forward 9/7 (ICT)  R' = (float)R - (float)off; c_k = fmaf(m_k2, B', fmaf(m_k1, G', m_k0 * R')), the matrix and
 *                           order of the 8-bit transform.
 *        inverse 5/3        G' = c0 - ((c1 + c2) >> 2), R' = c2 + G', B' = c1 + G'; sample = clamp(x + off, 0, mx).
 *        inverse 9/7        x = (int)rintf(fmaf(M_k2, c2, fmaf(M_k1, c1, M_k0 * c0)) + 0.01f); sample = clamp(x + off, 0, mx):
 *                           the 8-bit arithmetic with 255 replaced by mx (a NaN component is left unspecified).
 *      Samples are read UNSIGNED; one above mx is the caller's error: coded as it is, decoded clamped.  Component c is
 *      then a deep grey plane coded with table c (32-bit coefficients, one launch a stage over the 3 n planes, plane z
 *      with table z % 3).  Header: both depth fields carry bd, components 3, is_rgb 1, n_samples = W * H * 3.
 *      picsong_ctx_set_decode_drop stays allowed: the three components use the same drop.
 *      Range: the RCT's chroma components span +-(2^bd - 1), one bit more than a grey sample; the ICT's rows have absolute
 *      sum 1, so |c_k| <= off.  picsong_depth_range_guaranteed_rgb (host only): the bound of
 *      picsong_depth_range_guaranteed with max|sample| = 2^bd for 5/3 and 2^(bd-1) for 9/7; refuses what that call
 *      refuses and bit_depth 8.  Where it says no the calls do not refuse: a coefficient that reaches 2^15 raises
 *      picsong_range_flag, as on a deep grey context.
 *      picsong_rgb_forward16 / picsong_rgb_inverse16: the stage seams, uint16[P] x 3 <-> T[P] x 3 (T = int32 / float);
 *        the sample pointers need 2-byte alignment (8-byte aligned ones take one 8-byte access a lane's four samples,
 *        others 2-byte accesses: the same values); the T planes 16-byte alignment (refused otherwise).
 *      picsong_encode_rgb_frames16 / picsong_decode_rgb_frames16: n = 1..21 frames.  d_r / d_g / d_b are frame 0's
 *        planes, frame f's lie f * frame_stride BYTES after each; frame_stride is even, >= 2 P, must not let a frame's
 *        planes overlap the next frame's, and is ignored for n = 1.  Streams at (3 f + c) * stream_stride shorts;
 *        first_iter, header_mask, lengths and asynchrony exactly as picsong_encode_rgb_frames /
 *        picsong_decode_rgb_frames; -cp 2 only, any -k; the three tables must share one geometry.  One launch a
 *        transform level over the 3 n planes (grid.z = plane).  Encoding, level 0 reads a frame's three sample planes
 *        and applies the colour transform in its load stage, so the component planes are never written: its vector
 *        form (three 8-byte loads a lane) where all three planes are 16-byte aligned and frame_stride is a multiple
 *        of 16, its per-column form otherwise; PICSONG_DEEP_NOFUSE=1 (read per call) runs the colour transform of the
 *        n frames as ONE launch of its own (grid.y = frame) and the T-input level 0 instead: the same bytes.
 *        Decoding, the synthesis writes the 3 n T planes and ONE inverse-transform launch follows.  Every stream is
 *        byte-identical to picsong_rgb_forward16 + 3 x picsong_encode_plane of that frame, every decoded plane to
 *        3 x picsong_decode_plane + picsong_rgb_inverse16.  Decoding writes exactly 2 P bytes a plane.  Pointers
 *        need 2-byte alignment.
 *      picsong_image layouts PLANAR3_16, RGB48 and RGBA64 (native uint16 samples): data, pitch and the strides are
 *        2-byte aligned (refused otherwise), pitch >= W * bpp (2, 6, 8); no byte outside [y * pitch, y * pitch + W * bpp)
 *        of rows 0 .. H - 1 is read or written; RGBA64's A is ignored on input and written as mx on output.
 *        picsong_ingest_frames / picsong_emit_frames accept them on a deep RGB context: the padded side is three
 *        uint16 planes a frame (R, G, B, 2 P bytes each), passed through the uint8_t * parameter, padded_stride in
 *        bytes (>= 6 P).  picsong_encode_rgb_images / picsong_decode_rgb_images accept them there: ONE ingest (emit)
 *        of the n frames into (from) the context's aligned buffer, then the frame calls above, byte-identical to them
 *        on host-padded planes.  A 4-byte aligned image side and a 16-byte aligned padded side take the vector form
 *        (dwords of the image, a dwordx4 a plane), anything else 2-byte accesses: the same bytes.  They are refused on
 *        every other context; the 8-bit layouts and GREY16 are refused on a deep RGB context.
 *      Refused on a deep RGB context (PICSONG_ERR_ARG, nothing launched, outputs untouched): every call that takes or
 *      returns uint8_t frames, the 8-bit RGB calls included; picsong_encode_frames16 / picsong_decode_frames16; the
 *      searches, training on frames, the uint8_t proxies ("deep proxies" below are the uint16 ones) and stripes;
 *      picsong_encode_images / picsong_decode_images and the single-frame picsong_encode_rgb_image /
 *      picsong_decode_rgb_image.  The plane calls (picsong_encode_plane,
 *      picsong_decode_plane and the stage calls on T arrays) work as on a deep grey context.  Refused on every other
 *      context: the four device calls below.
 *      Not built: a fused tail for the decode, bgr / bgra 16-bit layouts. ---- */
int picsong_depth_range_guaranteed_rgb(int bit_depth, int lossy, int wl, float qs, int *yes);          /* host only */
int picsong_rgb_forward16(picsong_ctx *ctx, const uint16_t *d_r, const uint16_t *d_g, const uint16_t *d_b, void *d_c0,
                          void *d_c1, void *d_c2, void *stream);
int picsong_rgb_inverse16(picsong_ctx *ctx, const void *d_c0, const void *d_c1, const void *d_c2, uint16_t *d_r,
                          uint16_t *d_g, uint16_t *d_b, void *stream);
int picsong_encode_rgb_frames16(picsong_ctx *ctx, int n, const uint16_t *d_r, const uint16_t *d_g, const uint16_t *d_b,
                                size_t frame_stride, int first_iter, int header_mask,
                                uint16_t *d_streams, size_t stream_stride, void *stream);
int picsong_decode_rgb_frames16(picsong_ctx *ctx, int n, const uint16_t *d_streams, size_t stream_stride,
                                uint16_t *d_r, uint16_t *d_g, uint16_t *d_b, size_t frame_stride, void *stream);

/* ---- colour proxies: n = 1..21 RGB frames at 1/2^reduce, or a window of them, through ONE launch per stage over the
 *      3 n planes -- thumbnails, previews and editing proxies of a colour video, whose launches are too small to run
 *      one frame a call.  Streams as picsong_decode_rgb_frames reads them: frame f, component c at d_streams +
 *      (3 f + c) * stream_stride shorts.  Asynchronous on `stream`; -cp 2 RGB contexts, any -k, 5/3 and 9/7, reduce in
 *      0..wl-1; picsong_range_flag covers the codeblocks a call decodes; the context grows its batch workspace to 3 n
 *      planes.  frame_stride is ignored for n = 1.
 *      picsong_decode_rgb_frames_reduced: frame f's planes, paw x pah bytes each (picsong_reduced_dims), at d_r / d_g /
 *      d_b + f * frame_stride, byte-identical to picsong_decode_rgb_frame_reduced of that frame; no byte beyond them is
 *      written; reduce = 0 is picsong_decode_rgb_frames.  Planes and frame_stride 4-byte aligned take the fused tail
 *      (finest synthesis level + inverse RCT / ICT in one launch, grid.z = frame) where the single-frame call takes it,
 *      anything else the separate inverse colour transform (one launch a frame).
 *      picsong_decode_rgb_frames_window: frame f's three windows, byte-identical to picsong_decode_rgb_frame_window; row
 *      i goes to d_x + f * frame_stride + i * out_pitch, w bytes, and nothing else is written.  Any alignment.  Only the
 *      codeblocks of the window's cone are decoded (picsong_window_codeblocks: per frame and component).
 *      picsong_decode_rgb_images_window: the same windows in a colour layout of picsong_image -- PLANAR3, RGB24, BGR24,
 *      RGBA32, BGRA32 --: pixel (j, i) of frame f's window at dst->data + f * frame_stride + i * dst->pitch + j * bpp,
 *      alpha 255; no byte outside [i * pitch, i * pitch + w * bpp) of rows 0..h-1 is written.  The bytes are those of
 *      picsong_decode_rgb_frames_window interleaved as picsong_emit_frames interleaves; the epilogue kernel writes the
 *      layout itself (dword / dwordx4 stores where data, pitch and frame_stride are 4-byte aligned, per byte otherwise).
 *      picsong_decode_rgb_images_reduced: the visible rw x rh pixels (picsong_reduced_dims) of each frame at
 *      1/2^reduce, the bytes of picsong_decode_rgb_images_window with the window (0, 0, rw, rh).  Where paw is a
 *      multiple of 16 it runs picsong_decode_rgb_frames_reduced into the context's aligned buffer and ONE emit of the
 *      n frames (the faster route: 16-bit coefficients, the fused tail), else that window call.
 *      Refused (PICSONG_ERR_ARG, nothing launched, outputs untouched): null pointers; a grey context; -cp 3; n outside
 *      1..21; reduce outside 0..wl-1; a stream stride below a worst-case stream; component tables of different
 *      geometry.  The frames calls with n > 1: a frame_stride below one plane's span (paw * pah; (h - 1) * out_pitch +
 *      w) or one that makes a frame's planes overlap the next frame's.  The window calls: everything
 *      picsong_decode_rgb_frame_window refuses.  The image calls: an unknown layout or GREY8, pitch < w * bpp, a
 *      PLANAR3 plane_stride below a plane's span, with n > 1 a frame_stride below a frame's span. ---- */
int picsong_decode_rgb_frames_reduced(picsong_ctx *ctx, int n, const uint16_t *d_streams, size_t stream_stride, int reduce,
                                      uint8_t *d_r, uint8_t *d_g, uint8_t *d_b, size_t frame_stride, void *stream);
int picsong_decode_rgb_frames_window(picsong_ctx *ctx, int n, const uint16_t *d_streams, size_t stream_stride, int reduce,
                                     int x, int y, int w, int h, uint8_t *d_r, uint8_t *d_g, uint8_t *d_b,
                                     size_t out_pitch, size_t frame_stride, void *stream);
int picsong_decode_rgb_images_reduced(picsong_ctx *ctx, int n, const uint16_t *d_streams, size_t stream_stride, int reduce,
                                      const picsong_image *dst, size_t frame_stride, void *stream);
int picsong_decode_rgb_images_window(picsong_ctx *ctx, int n, const uint16_t *d_streams, size_t stream_stride, int reduce,
                                     int x, int y, int w, int h, const picsong_image *dst, size_t frame_stride, void *stream);

/* ---- deep proxies: the reduced and the window decode of 9- to 16-bit frames, grey and RGB -- thumbnails and regions of
 *      cinema, broadcast, medical and remote-sensing masters without decoding the whole frame at 32-bit coefficients.
 *      The four calls mirror picsong_decode_frames_reduced / _window and picsong_decode_rgb_frames_reduced / _window on
 *      native (little-endian) uint16_t samples; asynchronous on `stream`.  What changes:
 *        the level shift and clamp are the deep context's (off = 2^(bd-1), mx = 2^bd - 1): 5/3 clamp(v + off, 0, mx);
 *        9/7 clamp(rintf((v + off) + 0.01f), 0, mx), NaN -> 0; RGB the inverse RCT / ICT of "deep RGB contexts" above,
 *        applied to the three components' LL_reduce.
 *        frame_stride and out_pitch are in BYTES and must be even; pointers need 2-byte alignment.
 *        Grey takes n = 1..64 (a deep grey context), RGB n = 1..21 (a deep RGB one); frame_stride is ignored for n = 1.
 *      The reduced calls write exactly paw * pah samples a plane (picsong_reduced_dims), row stride paw samples, and
 *      nothing else; reduce = 0 is byte-identical to picsong_decode_frames16 / picsong_decode_rgb_frames16.  The window
 *      calls write the w samples of row i at (char *)d_out + f * frame_stride + i * out_pitch and nothing else; a window is
 *      byte for byte that rectangle of the reduced call's output.  Only the codeblocks of the corner or of the window's
 *      cone are decoded (picsong_window_codeblocks); picsong_range_flag covers those.  picsong_ctx_set_decode_drop
 *      composes as on 8-bit contexts.  -cp 2 only, any -k, 5/3 and 9/7, the 32-bit coefficient form.
 *      Forms, always the same bytes.  Grey reduced: the level-`reduce` launch stores the samples itself where the output
 *      and frame_stride are 16-byte aligned and PICSONG_DEEP_NOFUSE is unset, else a clamp pass a frame.  RGB reduced:
 *      the synthesis of the 3 n planes, then ONE inverse-transform launch over the n frames.  Grey window: level r of the
 *      cone stores the samples.  RGB window: one epilogue launch (grid.z = frame) that reads the three components' T
 *      samples, four pixels a thread, and stores dwords (dwordx2 where 8-byte aligned) where pointers, pitch and
 *      frame_stride are 4-byte aligned, single samples otherwise and in a row's last partial group.
 *      picsong_decode_rgb_images_window / picsong_decode_rgb_images_reduced accept PLANAR3_16, RGB48 and RGBA64 on a deep
 *      RGB context: data, pitch, plane_stride and frame_stride 2-byte aligned, pitch >= w * bpp (2, 6, 8), alpha written
 *      as mx, no byte outside [i * pitch, i * pitch + w * bpp) of rows 0..h-1 written; the epilogue writes the layout
 *      itself.  _reduced yields the visible rw x rh samples through the window (0, 0, rw, rh) -- the only route on a deep
 *      context.  The 8-bit layouts stay refused on a deep RGB context, the 16-bit ones on every other context.
 *      picsong_reduced_dims and picsong_window_codeblocks answer on deep contexts (geometry only).
 *      Refused (PICSONG_ERR_ARG, nothing launched, outputs untouched; the message names the call to use instead where the
 *      context is of another kind): the four calls on an 8-bit context; the grey pair on a deep RGB context and the RGB
 *      pair on a deep grey one; -cp 3; null pointers; n out of range; reduce outside 0..wl-1; a window not inside
 *      paw x pah or with w or h < 1; odd pointers, pitches or strides; out_pitch < 2 w; with n > 1 a frame_stride below
 *      a plane's span (2 paw pah; (h - 1) * out_pitch + 2 w) or, RGB, one that makes a frame's planes overlap the next
 *      frame's; a stream stride below picsong_max_stream_shorts (grey: with n > 1); component tables of different
 *      geometry.  The uint8_t proxy calls stay refused on deep contexts.
 *      Not built: 8-bit output from deep streams, bgr / bgra 16-bit layouts, the int16 coefficient form,
 *      a fused deep RGB tail, the CLI flags. ---- */
int picsong_decode_frames16_reduced(picsong_ctx *ctx, int n, const uint16_t *d_streams, size_t stream_stride, int reduce,
                                    uint16_t *d_frames_out, size_t frame_stride, void *stream);
int picsong_decode_frames16_window(picsong_ctx *ctx, int n, const uint16_t *d_streams, size_t stream_stride, int reduce,
                                   int x, int y, int w, int h, uint16_t *d_out, size_t out_pitch, size_t frame_stride, void *stream);
int picsong_decode_rgb_frames16_reduced(picsong_ctx *ctx, int n, const uint16_t *d_streams, size_t stream_stride, int reduce,
                                        uint16_t *d_r, uint16_t *d_g, uint16_t *d_b, size_t frame_stride, void *stream);
int picsong_decode_rgb_frames16_window(picsong_ctx *ctx, int n, const uint16_t *d_streams, size_t stream_stride, int reduce,
                                       int x, int y, int w, int h, uint16_t *d_r, uint16_t *d_g, uint16_t *d_b,
                                       size_t out_pitch, size_t frame_stride, void *stream);

/* ---- intra-frame sharding (BASELINE config 5): codeblocks are independent
 *      (correctCBBorders zeroes outside neighbours, BPC/BPCEngine.cu:465-484), so a rank can code
 *      the stripe [cb_begin, cb_begin + cb_count) of the frame's raster-ordered codeblocks.  The
 *      stripe leaves as a self-describing mini-stream with the normal layout for cb_count blocks:
 *      9 x 0xFFFF | cb_count x (MSB, len) | payload | 0xFFFF.  The writer rank splices: header(9) +
 *      all pair tables in stripe order + all payloads in stripe order + 0xFFFF == the 1-GPU
 *      stream.  The DWT is computed for the whole frame on every rank (it needs all rows).
 *      Asynchronous; length via picsong_last_total(). ---- */
int picsong_encode_frame_stripe(picsong_ctx *ctx, const uint8_t *d_frame, int cb_begin, int cb_count,
                                uint16_t *d_stream, void *stream);
/* Row-band sharding of the transform for the same split ("partition level 0 by row bands
 * with a halo of 2 (5/3) or 4 (9/7) rows per side ... then all-gather LL1 and compute levels >= 1
 * redundantly"): no rank transforms or even holds the whole frame.
 *   picsong_dwt_forward_band: level 0 (u8 ingest, level shift fused) of the input rows [row0, row0 + rows)
 *     only -- row0 and rows even; d_frame is addressed in frame coordinates (row y at d_frame + y * AW) but
 *     only the band's rows and its halo need to be present.  Writes rows [row0/2, (row0+rows)/2) of HL, LH and
 *     HH into the Mallat array at d_out and of LL1 into the scratch behind it (d_out + AW*AH elements, row
 *     stride AW/2) -- the same places picsong_dwt_forward_u8 writes them (DWTEngine::DWTForward's buffer
 *     contract, DWT/DWTGenerator.cu:1268-1342).
 *   picsong_dwt_forward_tail: levels 1 .. wl-1 from the complete LL1 in that scratch (after the ranks have
 *     all-gathered their LL1 row bands in place).
 *   picsong_encode_stripe_coded: coder + pack of the codeblocks [cb_begin, cb_begin + cb_count) from a
 *     coefficient array (picsong_encode_frame_stripe without its transform); mini-stream as above.
 * With N ranks and AH a multiple of 128 N, rank k transforms input rows [k AH/N, (k+1) AH/N) and codes the
 * codeblock rows [k R, (k+1) R) and [AH/128 + k R, ...), R = AH / (128 N): exactly the coefficients its own
 * band and the shared tail produce.  Asynchronous. */
int picsong_dwt_forward_band(picsong_ctx *ctx, const uint8_t *d_frame, int row0, int rows, void *d_out,
                             void *stream);
int picsong_dwt_forward_tail(picsong_ctx *ctx, void *d_out, void *stream);
int picsong_encode_stripe_coded(picsong_ctx *ctx, const void *d_coeffs, int cb_begin, int cb_count,
                                uint16_t *d_stream, void *stream);
/* host helper: IOManager::loadFrameCAdaptedSizes' mirror padding (IO/IOManager.ipp:72-112).
 * PICSONG_ERR_ARG when aw - w > w or ah - h > h: the reference's loop is undefined there. */
int picsong_pad_frame_host(const uint8_t *in, int w, int h, uint8_t *out, int aw, int ah);

/* ---- measurement: per-stage durations of picsong_encode_frame, taken with HIP events recorded
 *      on the launch stream (the reference accumulates host chrono time around its BPC kernel,
 *      BPC/BPCEngine.cu:2318-2422, "BPC acum time").  profile_begin(capacity) arms a ring of event
 *      sets; every later encode_frame records into the next set without synchronising;
 *      profile_read synchronises the last set and returns, per recorded frame, 3 floats:
 *      {dwt_ms (all levels), bpc_ms (bpc_kernel), pack_ms (scan + pack)}.  capacity 0 disarms.
 *      A quality call (picsong_encode_frame_quality and its mirrors) records one set per PROBE instead:
 *      {quantise_ms, synthesis_ms, sse_ms}. ---- */
int picsong_profile_begin(picsong_ctx *ctx, int capacity);
int picsong_profile_read(picsong_ctx *ctx, int *n_frames, float *ms, int ms_capacity_frames);

/* ---- self-test of the hardware property the coder's slot reservation uses (one LDS atomic add per
 *      codeword; lanes of one instruction that hit one counter are served in ascending lane order, the
 *      order of arithmeticEncoder's __activemask reservation, BPC/BPCEngine.cu:380-393): 16 M random lane
 *      masks against the v_mbcnt ranks.  *mismatches must come back 0; a build with
 *      -DPICSONG_ENC_LDS_RESERVE=0 does not depend on it. ---- */
int picsong_selftest_lds_order(int device, int *mismatches);

/* ---- diagnostics: nonzero if, since the previous query (reading clears it), any codeblock of a
 *      bpc call on ctx had MSB > 15 (outside the LUT's 15 bit-planes), or if
 *      picsong_bitstream_unpack / picsong_decode_frame
 *      met a codeblock length outside 1..4096 (damaged stream: the length is clamped, so no access
 *      leaves the staging or 9 + 2n + 4095n + 1 shorts of the stream buffer); synchronises `stream`. ---- */
int picsong_range_flag(picsong_ctx *ctx, void *stream, int *h_flag);

#ifdef __cplusplus
}
#endif
#endif
