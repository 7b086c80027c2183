// PICSONG command-line tool for MI355X -- host side (C++) of the hot path, written over the C ABI
// of include/picsong_hip.h.  It keeps the reference's flags, defaults, validation, file formats and
// console vocabulary (Launcher.cu:8-29,36-163; IO/IOManager.ipp:72-112,176-231,267-344,615-620) so
// it is a drop-in for the greyscale and RGB (planar R,G,B; RCT / ICT) image / video encode + decode
// paths, including the complexity-scalable mode -k > 0 and the three-coding-pass mode -cp 3 (deprecated in
// the reference, whose tree ships no cp_sig / cp_sign tables for it: -LUTFolder must hold them).
//
// Pipeline (grey video encode, run_encode): the reference's reader / worker / writer structure
// (CodingEngine.cu:212-262,463-498,758-1069) with condition variables instead of its spin-wait flag
// arrays (_doubleBufferInput/_doubleBufferOutput, :233-239).  A ring of slots, each with its own
// picsong_ctx, HIP stream, pinned host buffers and device buffers; a slot carries one GROUP of up to B
// consecutive frames (frames_per_launch), group g lives in slot g mod S (S = max(-numberOfStreams, 3) + 3,
// rounded up to a multiple of the devices).  Two reader threads stage the groups in the pinned input
// buffers (stage_frames), the main thread launches H2D copy + encode on the slot's stream (upload_frames),
// a collector thread waits for the groups' stream lengths in group order and fixes every frame's file
// offset, two writer threads copy the codestreams back and pwrite them; the _SIZE entries are appended in
// frame order at the end.  The grey video decode (run_decode_video) is a second, deliberately separate
// pipeline of the same shape without a collector: the _SIZE sidecar gives every offset up front.
// Everything else -- RGB, -train, -bps 9..16, still-image decode, -compare -- is straight-line code on one
// stream.  The file rules live in cli_io.hpp; device and pinned memory, streams and contexts are owned
// (Owned) and freed where their scope ends -- die() exits without unwinding.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/picsong_hip.h"
#include "cli_io.hpp"

namespace {

using namespace cli_io;

struct Options {
    std::string input, output, lut_folder;
    int cd = 2, x = 0, y = 0, cb_width = 64, cb_height = 18, wl = 5, cp = 2, endianess = 0, bps = 8;
    int signed_or_unsigned = 0, video = 0, frames = 0, avoid_size_check = 0, components = 1, streams = 2;
    int is_rgb = 0, type = 0, device = 0, lut_fill = 0;
    int gpus = 1, frames_per_launch = 0;        // -gpus N: frames sharded over N devices; -framesPerLaunch B (0 = by frame size)
    std::string devices;                        // --devices a,b,..: explicit device list (a device may repeat)
    float qs = 1.0f, k = 0.0f;
    std::string metrics;
    int reduce = 0;                             // -reduce r: decode the image at 1/2^r of its size
    int win = 0, wx = 0, wy = 0, ww = 0, wh = 0; // -window x,y,w,h: decode that rectangle of the image at 1/2^r
    int drop = 0;                               // -drop d: decode at reduced quality (picsong_ctx_set_decode_drop)
    int win_cb = 0;                             // (the codeblocks a window decodes, for --metrics)
    std::string train;                          // -train <outFolder>: count the input's coding decisions, write a LUT folder
    float rate = 0.0f;                          // -rate <bpp>: choose qs so that the output meets that many bits per pixel
    bool has_rate = false, has_qs = false;
    double psnr = 0.0;                          // -psnr <dB>: choose qs so that the searched frames decode to at least that PSNR
    bool has_psnr = false;
    double ssim = 0.0;                          // -ssim <v>: choose qs so that the searched frames decode to at least that SSIM
    bool has_ssim = false;
    bool has_quality() const { return has_psnr || has_ssim; }   // a search that measures the decode: -psnr or -ssim
    int search_frames = 0;                      // -searchFrames N: the frames of a video the -rate / -psnr search runs on (0: the default)
    std::string compare;                        // -compare <raw file>: decoding, the PSNR of the output against that file
    int layout = -1;                            // -layout: the pixel layout of the raw file (PICSONG_LAYOUT_*), -1: not given
};

[[noreturn]] void die(const std::string &msg)
{
    std::cout << msg << std::endl;
    std::exit(-1);
}

#define CK(expr)                                                                        \
    do {                                                                                \
        int rc_ = (expr);                                                               \
        if (rc_ != PICSONG_OK) die(std::string(#expr) + " failed: " + picsong_last_error()); \
    } while (0)
#define HIPCK(expr)                                                                     \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) die(std::string(#expr) + " failed: " + hipGetErrorString(e_)); \
    } while (0)

// ---- owners of device memory, pinned memory, a stream and a context: move-only, released by the destructor
template <typename H, auto Release> struct Owned {
    H p = nullptr;
    Owned() = default;
    Owned(Owned &&o) noexcept : p(o.p) { o.p = nullptr; }
    Owned &operator=(Owned &&o) noexcept { std::swap(p, o.p); return *this; }
    ~Owned() { if (p) (void)Release(p); }
    operator H() const { return p; }
};
template <typename T> using Dev = Owned<T *, hipFree>;
template <typename T> using Pinned = Owned<T *, hipHostFree>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Ctx = Owned<picsong_ctx *, picsong_ctx_destroy>;       // (picsong_ctx_destroy makes the context's device current itself)
template <typename T> Dev<T> dev_alloc(size_t bytes) { Dev<T> b; HIPCK(hipMalloc(&b.p, bytes)); return b; }
template <typename T> Pinned<T> pinned_alloc(size_t bytes) { Pinned<T> b; HIPCK(hipHostMalloc(&b.p, bytes)); return b; }
Stream stream_create() { Stream s; HIPCK(hipStreamCreate(&s.p)); return s; }

// flag lookup: the value is the token after the flag (IO/CommandLineParser.cpp:10-25)
struct Args {
    std::vector<std::string> t;
    Args(int argc, char **argv) { for (int i = 1; i < argc; i++) t.emplace_back(argv[i]); }
    bool has(const std::string &f) const { for (auto &s : t) if (s == f) return true; return false; }
    std::string get(const std::string &f) const
    {
        for (size_t i = 0; i + 1 < t.size(); i++) if (t[i] == f) return t[i + 1];
        return "";
    }
};

void help()
{
    std::cout <<
        "PICSONG (MI355X build) -- wavelet image / video codec, DWT + BPC-PaCo hot path on gfx950\n"
        " -cd 0|1            0 = code, 1 = decode\n"
        " -i <file> -o <file> input / output\n"
        " -xSize W -ySize H   frame dimensions (coding; optional when the input is a P5 PGM)\n"
        " -wl N               wavelet levels (1..7, default 5)\n"
        " -type 0|1           0 = lossless 5/3, 1 = lossy 9/7 (+ -qs in (0,1])\n"
        " -cp 2|3             coding passes (3: deprecated in the reference; needs cp_sig / cp_sign tables in -LUTFolder)\n"
        " -cbWidth 64 -cbHeight 18  kept for header compatibility\n"
        " -video 0|1 -frames F  video mode (raw planar frames; output + <o>_SIZE sidecar)\n"
        " -LUTFolder <dir>    probability tables (header.txt, {ref,sig,sign}R.txt_0)\n"
        " -numberOfStreams N  frames in flight (default 2)\n"
        " -isRGB 1 -components 3  planar R,G,B planes per frame (RCT lossless / ICT lossy)\n"
        " -k 0..65.535        complexity-scalable factor (needs the bit-plane LUT files _0.._14)\n"
        " -bps 8..16          bits a sample (default 8).  9..16: ONE grey still image -- coding reads a raw file of W*H\n"
        "                     little-endian 16-bit samples or a P5 PGM with maxval > 255 (big-endian samples), decoding\n"
        "                     writes a P5 with maxval 2^bps - 1.  With -isRGB 1 -components 3: one RGB still image or a video\n"
        "                     (-video 1 -frames F, -framesPerLaunch 1..21) of raw little-endian 16-bit samples, -layout planar\n"
        "                     (default: R, G, B planes of W*H), rgb (6 bytes a pixel) or rgba (8 bytes a pixel), in and out.\n"
        "                     -drop works; no grey video, -rate, -psnr, -ssim, -train, -reduce, -window, -gpus, -cp 3, -compare,\n"
        "                     and no -layout bgr / bgra\n"
        " -device D           GPU index (default 0);  --metrics <file>  JSON stage timings\n"
        " -gpus N             video coding: groups of frames sharded round-robin over devices D .. D+N-1 of this node\n"
        "                     (--devices a,b,c names them explicitly); every device copies its codestreams to the\n"
        "                     writer's pinned ring over its own host link, the output file is the 1-GPU file\n"
        " -framesPerLaunch B  frames coded / decoded per launch (default: 4 up to 4K frames, 1 above; an RGB video:\n"
        "                     the same rule on a frame's three planes -- decoding with -reduce / -window: on the three\n"
        "                     planes it writes -- at most 21)\n"
        " --lut-fill V        value of LUT entries the loader never writes (default 0)\n"
        " -reduce r           decoding: the image at 1/2^r of its size, r in 0..wl-1 (resolution reduction); an RGB video\n"
        "                     goes through groups of -framesPerLaunch frames, as at full size (-window too)\n"
        " -window x,y,w,h     decoding: only the w x h rectangle at (x, y) of the image (at 1/2^r with -reduce r), from the\n"
        "                     codeblocks it depends on (spatial random access)\n"
        " -drop d             decoding, -cp 2 streams coded at -k 0: the image at its full size from fewer bit-planes, d in 0..15\n"
        "                     (quality reduction): a codeblock of wavelet level l (0 the finest) leaves its max(0, d - l)\n"
        "                     lowest bit-planes undecoded, the coder's most expensive ones.  With -reduce, -window, -video,\n"
        "                     -isRGB, -framesPerLaunch, -layout and -compare (the PSNR of the quick decode)\n"
        " -train <outFolder>  coding (-cd 0, -cp 2, -k 0): code nothing; count the input's coding decisions and write the\n"
        "                     probability tables fitted to them as a LUT folder for this -wl (no -o needed).  -LUTFolder,\n"
        "                     if given, is the prior: its geometry, and its values for entries the input never reaches\n"
        " -rate <bpp>         coding, -type 1: choose -qs so that a frame takes at most bpp bits per pixel (floor(bpp W H / 16)\n"
        "                     shorts; an RGB frame's three components share it).  A video gets ONE qs (its stream has one header):\n"
        "                     the search runs on the first min(frames, 16) frames and their summed target, the whole video is\n"
        "                     coded at the result.  Not with -qs, -type 0 or -cp 3\n"
        " -psnr <dB>          coding, -type 1: choose -qs so that the PSNR over the visible samples of the searched frames is at\n"
        "                     least dB (an SSE of at most floor(65025 samples / 10^(dB/10)), samples = W H frames components).  A\n"
        "                     video as with -rate: the search runs on the first min(frames, 16) frames (an RGB video: its first\n"
        "                     frame).  Not with -qs, -rate, -type 0, -cp 3 or -train\n"
        " -ssim <v>           coding, -type 1: choose -qs so that the SSIM (x264's integer 8 x 8 measure, windows every 4 samples)\n"
        "                     over the searched frames is at least v, 0 < v <= 1: a DSSIM sum of at most\n"
        "                     floor((1 - v) windows 2^24), windows = ((W - 8) / 4 + 1) ((H - 8) / 4 + 1) frames components; W and\n"
        "                     H 8 or more.  A video as with -psnr.  Not with -qs, -rate, -psnr, -type 0, -cp 3 or -train\n"
        " -searchFrames N     coding, -video 1 with -rate, -psnr or -ssim: the search runs on the first min(N, frames) frames -- grey\n"
        "                     N = 1..16, an RGB video N = 1..21 (one search call over the N colour frames, whose streams are\n"
        "                     the search's own output).  Without it: grey min(frames, 16), an RGB video its first frame\n"
        " -compare <file>     decoding: after the output is written, print its PSNR and SSE (and, from 8 x 8 samples on, its SSIM\n"
        "                     and DSSIM sum) against that raw (or PGM) file of the same geometry and planar layout.  Not with\n"
        "                     -reduce or -window\n"
        " -layout grey|planar|rgb|bgr|rgba|bgra\n"
        "                     the pixel layout of the raw file: the input's when coding, the output's when decoding; rows of\n"
        "                     W * bpp bytes (1, 1, 3, 3, 4, 4 bytes a pixel; planar: the R, G, B planes one after the other;\n"
        "                     alpha is ignored when coding and written as 255 when decoding).  grey for -components 1, the\n"
        "                     others for -isRGB 1.  The frame is then uploaded as it is and padded / split (cropped /\n"
        "                     interleaved) on the GPU: no host pass.  grey and planar give the files the flag's absence\n"
        "                     gives.  Not with -reduce, -window, -train or (interleaved layouts) -compare\n";
}

template <typename T> void echo(const char *flag, const T &v)
{
    std::cout << "User entered " << flag << " command " << v << std::endl;
}

Options parse(const Args &a)
{
    Options o;
    auto geti = [&](const char *f, int &dst) { if (a.has(f)) { dst = std::stoi(a.get(f)); echo(f, dst); } };
    auto getf = [&](const char *f, float &dst) { if (a.has(f)) { dst = std::stof(a.get(f)); echo(f, dst); } };
    auto gets = [&](const char *f, std::string &dst) { if (a.has(f)) { dst = a.get(f); echo(f, dst); } };
    geti("-cd", o.cd);
    gets("-i", o.input); gets("-o", o.output); gets("-LUTFolder", o.lut_folder);
    geti("-numberOfStreams", o.streams); geti("-video", o.video);
    geti("-device", o.device); geti("--lut-fill", o.lut_fill); gets("--metrics", o.metrics);
    geti("-gpus", o.gpus); geti("-framesPerLaunch", o.frames_per_launch); gets("--devices", o.devices);
    geti("-reduce", o.reduce);
    if (a.has("-reduce") && o.cd != 1) die("Incorrect parameters. -reduce applies to decoding (-cd 1) only.");
    if (a.has("-drop")) {
        if (o.cd != 1) die("Incorrect parameters. -drop applies to decoding (-cd 1) only.");
        geti("-drop", o.drop);
        if (o.drop < 0 || o.drop > 15) die("Incorrect parameters. -drop takes a number of bit-planes in 0..15.");
    }
    if (a.has("-window")) {
        if (o.cd != 1) die("Incorrect parameters. -window applies to decoding (-cd 1) only.");
        const std::string v = a.get("-window");
        char tail = 0;
        if (sscanf(v.c_str(), "%d,%d,%d,%d%c", &o.wx, &o.wy, &o.ww, &o.wh, &tail) != 4 || o.wx < 0 || o.wy < 0 || o.ww < 1 ||
            o.wh < 1)
            die("Incorrect parameters. -window takes x,y,w,h: x, y >= 0, w, h >= 1.");
        o.win = 1;
        echo("-window", v);
    }
    // a flag of coding only; -psnr / -ssim: a number read whole (strtod), echoed as given
    auto coding_only = [&](const char *f) {
        if (a.has(f) && o.cd != 0) die(std::string("Incorrect parameters. ") + f + " applies to coding (-cd 0) only.");
        return a.has(f);
    };
    auto getd = [&](const char *f, double &dst, bool &given, bool (*ok)(double), const char *takes) {
        const std::string v = a.get(f);
        char *end = nullptr;
        dst = std::strtod(v.c_str(), &end);
        given = true;
        if (v.empty() || *end != '\0' || !ok(dst)) die(std::string("Incorrect parameters. ") + f + " takes " + takes);
        echo(f, v);
    };
    if (coding_only("-train")) {
        gets("-train", o.train);
        if (o.train.empty()) die("Incorrect parameters. -train takes the folder to write.");
    }
    if (coding_only("-rate")) {
        getf("-rate", o.rate);
        o.has_rate = true;
        if (!(o.rate > 0.0f)) die("Incorrect parameters. -rate takes a positive number of bits per pixel.");
    }
    if (coding_only("-psnr")) getd("-psnr", o.psnr, o.has_psnr, [](double v) { return std::isfinite(v); }, "a PSNR in dB.");
    if (coding_only("-ssim")) getd("-ssim", o.ssim, o.has_ssim, [](double v) { return v > 0.0 && v <= 1.0; }, "an SSIM above 0 and at most 1.");
    if (coding_only("-searchFrames")) {
        geti("-searchFrames", o.search_frames);
        if (o.search_frames < 1) die("Incorrect parameters. -searchFrames takes a number of frames, 1 or more.");
    }
    if (a.has("-compare")) {
        if (o.cd != 1) die("Incorrect parameters. -compare applies to decoding (-cd 1) only.");
        if (a.has("-reduce") || a.has("-window")) die("Incorrect parameters. -compare does not apply to -reduce or -window.");
        o.compare = a.get("-compare");
        if (o.compare.empty()) die("Incorrect parameters. -compare takes the file to compare with.");
        echo("-compare", o.compare);
    }
    if (a.has("-layout")) {
        static const char *const names[] = { "grey", "planar", "rgb", "bgr", "rgba", "bgra" };
        const std::string v = a.get("-layout");
        for (int i = 0; i < 6; i++) if (v == names[i]) o.layout = i;
        if (o.layout < 0) die("Incorrect parameters. -layout takes grey, planar, rgb, bgr, rgba or bgra.");
        if (a.has("-reduce") || a.has("-window")) die("Incorrect parameters. -layout does not apply to -reduce or -window.");
        if (a.has("-compare") && o.layout >= PICSONG_LAYOUT_RGB24) die("Incorrect parameters. -compare reads planar files: not with an interleaved -layout.");
        echo("-layout", v);
    }
    o.has_qs = a.has("-qs");
    if (o.cd == 0) {
        geti("-xSize", o.x); geti("-ySize", o.y); geti("-cbWidth", o.cb_width); geti("-cbHeight", o.cb_height);
        geti("-wl", o.wl); geti("-cp", o.cp); geti("-endianess", o.endianess); geti("-bps", o.bps);
        geti("-signedOrUnsigned", o.signed_or_unsigned); geti("-frames", o.frames);
        geti("-avoidSizeCheck", o.avoid_size_check); geti("-components", o.components);
        geti("-isRGB", o.is_rgb); geti("-type", o.type); getf("-qs", o.qs); getf("-k", o.k);
    }
    return o;
}

// ---- -layout: the raw file's frames as they are.  Bytes a pixel, bytes a frame of the file (rows of W * bpp bytes, planar:
// three planes), and the picsong_image of such a frame at a device address
int layout_bpp(int layout) { return layout < PICSONG_LAYOUT_RGB24 ? 1 : (layout < PICSONG_LAYOUT_RGBA32 ? 3 : 4); }
size_t layout_frame_bytes(int layout, int w, int h)
{
    return (size_t)w * (size_t)h * (size_t)layout_bpp(layout) * (layout == PICSONG_LAYOUT_PLANAR3 ? 3u : 1u);
}
picsong_image layout_image(int layout, void *d, int w, int h)
{
    picsong_image im;
    im.data = d; im.pitch = (size_t)w * (size_t)layout_bpp(layout); im.plane_stride = (size_t)w * (size_t)h; im.layout = layout;
    return im;
}
void layout_check_context(int layout, bool rgb)
{
    if (layout < 0) return;
    if (rgb != (layout != PICSONG_LAYOUT_GREY8))
        die(rgb ? "Incorrect parameters. -layout grey describes a one-component file: an RGB one is planar, rgb, bgr, rgba or bgra."
                : "Incorrect parameters. A one-component file is -layout grey (the colour layouts need -isRGB 1 -components 3).");
}

// ---- staging: frames [first, first + n) of `planes` planes each, from the raw file into the pinned h.  With -layout the
// frames as the file holds them, back to back; otherwise every plane padded on the host (picsong_pad_frame_host through
// `raw`, W * H bytes of scratch; a plane that needs no padding is read where it goes), P bytes a plane.  Returns the
// failure (empty: none)
const char *const kShortInput = "Input file is shorter than the requested frames.";
std::string stage_frames(const Options &o, int fd, size_t file_base, long first, int n, int planes, uint8_t *h, uint8_t *raw)
{
    if (o.layout >= 0) {
        const size_t fb = layout_frame_bytes(o.layout, o.x, o.y);
        return pread_exact(fd, h, fb * (size_t)n, file_base + (size_t)first * fb) ? "" : kShortInput;
    }
    const int aw = picsong_pad_dim(o.x), ah = picsong_pad_dim(o.y);
    const size_t P = (size_t)aw * ah, plane = (size_t)o.x * o.y;
    const bool padded_already = (o.x == aw && o.y == ah);
    for (int j = 0; j < n * planes; j++) {
        uint8_t *dst = h + (size_t)j * P;
        if (!pread_exact(fd, padded_already ? dst : raw, plane, file_base + ((size_t)first * planes + j) * plane)) return kShortInput;
        if (!padded_already && picsong_pad_frame_host(raw, o.x, o.y, dst, aw, ah) != PICSONG_OK) return picsong_last_error();
    }
    return "";
}
// ... and to the device: n staged frames into padded planes at d_pad, P bytes a plane; -layout: as they are to d_raw,
// padded and split there by picsong_ingest_frames
std::string upload_frames(const Options &o, picsong_ctx *ctx, hipStream_t s, const uint8_t *h, int n, int planes, uint8_t *d_raw, uint8_t *d_pad)
{
    const size_t P = (size_t)picsong_pad_dim(o.x) * picsong_pad_dim(o.y) * (size_t)planes;
    const size_t fb = o.layout >= 0 ? layout_frame_bytes(o.layout, o.x, o.y) : P;
    if (hipMemcpyAsync(o.layout >= 0 ? d_raw : d_pad, h, fb * (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess) return "HIP error in the frame upload";
    if (o.layout < 0) return "";
    const picsong_image im = layout_image(o.layout, d_raw, o.x, o.y);
    return picsong_ingest_frames(ctx, n, &im, fb, d_pad, P, s) == PICSONG_OK ? "" : picsong_last_error();
}

// ---- the streams a straight-line encode path writes: <o>, <o>_SIZE and the running total
struct StreamSink {
    std::ofstream out;
    SizeList sizes;
    long total_shorts = 0;
    explicit StreamSink(const std::string &o) : out(o, std::ios::binary | std::ios::app), sizes(o + "_SIZE") {}
};
// the n streams a call left `stride` shorts apart at d_out: back to back into the pinned h_out, one wait for the stream,
// then appended to the output, their lengths to _SIZE
void collect_streams(hipStream_t s, const uint16_t *d_out, size_t stride, const int *totals, int n, uint16_t *h_out, StreamSink &to)
{
    size_t at = 0;
    for (int j = 0; j < n; j++) {
        HIPCK(hipMemcpyAsync(h_out + at, d_out + (size_t)j * stride, (size_t)totals[j] * 2, hipMemcpyDeviceToHost, s));
        at += (size_t)totals[j];
        to.total_shorts += totals[j];
    }
    HIPCK(hipStreamSynchronize(s));
    to.out.write(reinterpret_cast<const char *>(h_out), (std::streamsize)(at * 2));
    to.sizes.append(totals, (size_t)n);
}

struct Worker {
    int device = 0;                                // the GPU this slot's context, stream and buffers live on
    Ctx ctx;
    Stream stream;
    Pinned<uint8_t> h_in;                          // padded frames, pinned / device
    Dev<uint8_t> d_in;
    Pinned<uint16_t> h_out;                        // codestreams, pinned / device
    Dev<uint16_t> d_out;
    std::vector<uint8_t> h_raw;                    // unpadded frame (host)
    Dev<uint8_t> d_raw;                            // -layout: the unpadded frames as read, on the device
    ~Worker() { (void)hipSetDevice(device); }      // ... and are released there
};

// component c uses the {ref,sig,sign}{R,G,B}.txt_0 files (Engine::initLUT Engines/Engine.cu:124-136);
// with k > 0 every bit-plane file _0 .. _(AMOUNT_OF_BITPLANE_FILES-1) (Engines/Engine.cu:12-56)
// -cp 3: the five sections ref, sig, sign, cp_sig, cp_sign of file _0 (IO/IOManager.ipp:539-606)
void load_lut(picsong_ctx *ctx, const Options &o, int wl, int components = 1, float k = 0.0f, int cp = 2)
{
    if (o.lut_folder.empty()) die("Incorrect parameters. Please choose valid values. (-LUTFolder is required)");
    const int n_tables = k > 0.0f ? 0 : 1;
    for (int c = 0; c < components; c++) {
        picsong_lut_info info;
        if (cp == 3) {
            CK(picsong_lut_load_cp(o.lut_folder.c_str(), c + 1, wl, o.lut_fill, 3, &info, nullptr, 0));
            std::vector<int32_t> table((size_t)info.n_ref + 2 * ((size_t)info.n_sig + info.n_sign));
            CK(picsong_lut_load_cp(o.lut_folder.c_str(), c + 1, wl, o.lut_fill, 3, &info, table.data(), table.size()));
            CK(picsong_ctx_set_lut_component(ctx, c, &info, table.data()));
            continue;
        }
        CK(picsong_lut_load_k(o.lut_folder.c_str(), c + 1, wl, o.lut_fill, n_tables, &info, nullptr, 0));
        std::vector<int32_t> table(((size_t)info.n_ref + info.n_sig + info.n_sign) * (size_t)info.n_tables);
        CK(picsong_lut_load_k(o.lut_folder.c_str(), c + 1, wl, o.lut_fill, n_tables, &info, table.data(), table.size()));
        CK(picsong_ctx_set_lut_component(ctx, c, &info, table.data()));
    }
}

picsong_params make_params(const Options &o)
{
    picsong_params p;
    memset(&p, 0, sizeof p);
    p.width = o.x; p.height = o.y; p.wl = o.wl; p.cp = o.cp; p.lossy = o.type ? 1 : 0; p.qs = o.qs; p.k = o.k;
    p.cb_width = o.cb_width; p.cb_height = o.cb_height; p.bit_depth = o.bps; p.frames = o.frames;
    p.components = o.components;
    p.is_rgb = o.is_rgb ? 1 : 0;
    return p;
}

// ---- -psnr <dB>: what the search chose and what it achieved (the two console lines; --metrics carries them too)
struct QualityReport { bool reported = false; int j = 0; float qs = 0; uint64_t max_sse = 0, sse = 0, samples = 0; long frames = 0; double psnr = 0; } g_quality;
struct SsimReport { bool reported = false; int j = 0; float qs = 0; uint64_t max_dssim = 0, dssim = 0, windows = 0; long frames = 0; double ssim = 0; } g_ssim;
long g_frames_searched = 0;             // the frames a -rate / -psnr search ran on (--metrics: "search_frames")

void write_metrics(const Options &o, const char *mode, long frames, double seconds, double dwt, double bpc,
                   double pack, long shorts)
{
    if (o.metrics.empty()) return;
    std::ofstream m(o.metrics, std::ios::trunc);
    m << "{\"mode\": \"" << mode << "\", \"frames\": " << frames << ", \"seconds\": " << seconds
      << ", \"mpixels_per_s\": " << (seconds > 0 ? (double)frames * o.x * o.y / seconds / 1e6 : 0.0)
      << ", \"dwt_ms\": " << dwt << ", \"bpc_ms\": " << bpc << ", \"pack_ms\": " << pack
      << ", \"stream_shorts\": " << shorts;
    // decoding: the size of the images written (1/2^reduce of the frame's, -reduce)
    if (std::string(mode).compare(0, 6, "decode") == 0)
        m << ", \"width\": " << o.x << ", \"height\": " << o.y << ", \"reduce\": " << o.reduce;
    if (g_quality.reported)
        m << ", \"psnr_target\": " << o.psnr << ", \"psnr_j\": " << g_quality.j << ", \"psnr_qs\": " << g_quality.qs
          << ", \"psnr_max_sse\": " << g_quality.max_sse << ", \"psnr_frames_searched\": " << g_quality.frames
          << ", \"psnr_sse\": " << g_quality.sse << ", \"psnr_achieved\": " << g_quality.psnr;
    if (g_ssim.reported)
        m << ", \"ssim_target\": " << o.ssim << ", \"ssim_j\": " << g_ssim.j << ", \"ssim_qs\": " << g_ssim.qs
          << ", \"ssim_max_dssim\": " << g_ssim.max_dssim << ", \"ssim_frames_searched\": " << g_ssim.frames
          << ", \"ssim_dssim\": " << g_ssim.dssim << ", \"ssim_achieved\": " << std::fixed << std::setprecision(6) << g_ssim.ssim
          << std::defaultfloat << std::setprecision(6);
    if (g_frames_searched > 0) m << ", \"search_frames\": " << g_frames_searched;
    if (o.win)
        m << ", \"window\": [" << o.wx << ", " << o.wy << ", " << o.ww << ", " << o.wh << "], \"codeblocks\": " << o.win_cb;
    m << "}\n";
}

// ---- -rate <bpp>: the target of one frame in shorts, floor(bpp * W * H / 16) (W x H unpadded; the three components of an
// RGB frame share it), and the two console lines
size_t rate_target_shorts(const Options &o)
{
    return (size_t)std::floor((double)o.rate * (double)o.x * (double)o.y / 16.0);
}
void rate_report_choice(int j, float qs, size_t target, long nframes_searched)
{
    g_frames_searched = nframes_searched;
    std::cout << "Rate control: qs " << qs << " (j = " << j << ") chosen for " << target << " shorts over " << nframes_searched
              << " frame(s)" << std::endl;
}
void rate_report_achieved(const Options &o, long total_shorts, long nframes)
{
    std::cout << "Rate control: achieved " << (double)total_shorts * 16.0 / ((double)o.x * o.y * (double)nframes)
              << " bits per pixel over the whole output (target " << o.rate << ")" << std::endl;
}
void quality_report(int j, float qs, uint64_t max_sse, uint64_t samples, long nframes_searched, const uint64_t *sse, int n)
{
    QualityReport &r = g_quality;
    g_frames_searched = nframes_searched;
    r.reported = true; r.j = j; r.qs = qs; r.max_sse = max_sse; r.samples = samples; r.frames = nframes_searched; r.sse = 0;
    for (int i = 0; i < n; i++) r.sse += sse[i];
    CK(picsong_sse_to_psnr(r.sse, samples, &r.psnr));
    std::cout << "Quality control: qs " << qs << " (j = " << j << ") chosen for an SSE of at most " << max_sse << " over "
              << nframes_searched << " frame(s)" << std::endl;
    std::cout << "Quality control: achieved " << r.psnr << " dB (SSE " << r.sse << ") over the frames searched" << std::endl;
}

// -ssim <v>: the limit over `planes` planes of the frame's geometry, and the two console lines
uint64_t ssim_limit(const Options &o, uint64_t planes, uint64_t &windows)
{
    uint64_t lim = 0;
    if (picsong_ssim_windows(o.x, o.y, &windows) != PICSONG_OK) die(std::string("-ssim: ") + picsong_last_error());
    windows *= planes;
    CK(picsong_ssim_to_dssim(o.ssim, windows, &lim));
    return lim;
}
std::string ssim_text(double v)
{
    std::ostringstream t;
    t << std::fixed << std::setprecision(6) << v;
    return t.str();
}
void ssim_report(int j, float qs, uint64_t max_dssim, uint64_t windows, long nframes_searched, const uint64_t *dssim, int n)
{
    SsimReport &r = g_ssim;
    g_frames_searched = nframes_searched;
    r.reported = true; r.j = j; r.qs = qs; r.max_dssim = max_dssim; r.windows = windows; r.frames = nframes_searched; r.dssim = 0;
    for (int i = 0; i < n; i++) r.dssim += dssim[i];
    CK(picsong_dssim_to_ssim(r.dssim, windows, &r.ssim));
    std::cout << "Quality control: qs = " << qs << " (j = " << j << ") chosen for a DSSIM sum of at most " << max_dssim << " over "
              << nframes_searched << " frame(s)" << std::endl;
    std::cout << "Quality control: achieved SSIM " << ssim_text(r.ssim) << " (DSSIM sum " << r.dssim << ")" << std::endl;
}

// ---- the search step of -rate / -psnr / -ssim: the search `o` asks for over an input on the device, into d_out; the choice and
// its console lines.  The input, by the family of library call it goes through: one padded grey frame (an image); n
// grey frames `stride` bytes apart; the R, G and B planes of one frame at d, d + stride and d + 2 * stride, coded with the
// header mask rgb_mask; or n such frames 3 * stride apart (-searchFrames on an RGB video).  The one-frame and n-frame
// calls set the search up differently in the library: n = 1 does not make them interchangeable here.  Returns the
// failure (empty: none); re-tuning contexts to the choice is the caller's.
enum SearchFamily { GREY_FRAME = 0, GREY_FRAMES = 1, RGB_FRAME = 2, RGB_FRAMES = 3 };
struct SearchInput { SearchFamily family; const uint8_t *d; size_t stride; int n, rgb_mask; };
struct SearchChoice { int j = 0; float qs = 0.0f; int totals[3 * 21] = { 0 }; };
std::string search_step(const Options &o, picsong_ctx *ctx, hipStream_t s, const SearchInput &in, uint16_t *d_out, size_t out_stride,
                        SearchChoice &r)
{
    const bool rgb = in.family >= RGB_FRAME;
    const int frames = in.n, arrays = rgb ? 3 * frames : frames;
    const uint8_t *g = in.d + in.stride, *b = g + in.stride;
    const size_t target = rate_target_shorts(o) * (size_t)frames;
    const uint64_t samples = (uint64_t)o.x * (uint64_t)o.y * (uint64_t)arrays;
    uint64_t lim = 0, sse[3 * 21] = { 0 };
    if (o.has_psnr && picsong_psnr_to_sse(o.psnr, samples, &lim) != PICSONG_OK) return std::string("-psnr: ") + picsong_last_error();
    uint64_t windows = 0;
    if (o.has_ssim) lim = ssim_limit(o, (uint64_t)arrays, windows);
    enum { SIZE = 0, PSNR = 1, SSIM = 2 };
    int rc = PICSONG_ERR_ARG;
    switch (in.family * 3 + (o.has_ssim ? SSIM : o.has_psnr ? PSNR : SIZE)) {
    case GREY_FRAME * 3 + SIZE: rc = picsong_encode_frame_rate(ctx, in.d, 0, target, 0, 0, d_out, s, &r.j, r.totals); break;
    case GREY_FRAME * 3 + PSNR: rc = picsong_encode_frame_quality(ctx, in.d, 0, lim, 0, 0, d_out, s, &r.j, r.totals, sse); break;
    case GREY_FRAME * 3 + SSIM: rc = picsong_encode_frame_ssim(ctx, in.d, 0, lim, 0, 0, d_out, s, &r.j, r.totals, sse); break;
    case GREY_FRAMES * 3 + SIZE: rc = picsong_encode_frames_rate(ctx, in.n, in.d, in.stride, 0, target, 0, 0, d_out, out_stride, s, &r.j, r.totals); break;
    case GREY_FRAMES * 3 + PSNR: rc = picsong_encode_frames_quality(ctx, in.n, in.d, in.stride, 0, lim, 0, 0, d_out, out_stride, s, &r.j, r.totals, sse); break;
    case GREY_FRAMES * 3 + SSIM: rc = picsong_encode_frames_ssim(ctx, in.n, in.d, in.stride, 0, lim, 0, 0, d_out, out_stride, s, &r.j, r.totals, sse); break;
    case RGB_FRAME * 3 + SIZE: rc = picsong_encode_rgb_frame_rate(ctx, in.d, g, b, in.rgb_mask, target, 0, 0, d_out, out_stride, s, &r.j, r.totals); break;
    case RGB_FRAME * 3 + PSNR: rc = picsong_encode_rgb_frame_quality(ctx, in.d, g, b, in.rgb_mask, lim, 0, 0, d_out, out_stride, s, &r.j, r.totals, sse); break;
    case RGB_FRAME * 3 + SSIM:       // (there is no one-frame call: n = 1 of the n-frame one, with no frame stride)
        rc = picsong_encode_rgb_frames_ssim(ctx, 1, in.d, g, b, 0, 0, in.rgb_mask, lim, 0, 0, d_out, out_stride, s, &r.j, r.totals, sse); break;
    case RGB_FRAMES * 3 + SIZE:
        rc = picsong_encode_rgb_frames_rate(ctx, in.n, in.d, g, b, 3 * in.stride, 0, in.rgb_mask, target, 0, 0, d_out, out_stride, s, &r.j, r.totals); break;
    case RGB_FRAMES * 3 + PSNR:
        rc = picsong_encode_rgb_frames_quality(ctx, in.n, in.d, g, b, 3 * in.stride, 0, in.rgb_mask, lim, 0, 0, d_out, out_stride, s, &r.j, r.totals, sse); break;
    case RGB_FRAMES * 3 + SSIM:
        rc = picsong_encode_rgb_frames_ssim(ctx, in.n, in.d, g, b, 3 * in.stride, 0, in.rgb_mask, lim, 0, 0, d_out, out_stride, s, &r.j, r.totals, sse); break;
    }
    if (rc == PICSONG_ERR_RATE) return std::string("-rate: no quantiser meets the target size (") + picsong_last_error() + ")";
    if (rc == PICSONG_ERR_QUALITY)
        return std::string(o.has_ssim ? "-ssim" : "-psnr") + ": no quantiser meets the target quality (" + picsong_last_error() + ")";
    if (rc != PICSONG_OK || picsong_rate_qs(r.j, &r.qs) != PICSONG_OK) return std::string("The quantiser search failed: ") + picsong_last_error();
    if (o.has_ssim) ssim_report(r.j, r.qs, lim, windows, frames, sse, arrays);
    else if (o.has_psnr) quality_report(r.j, r.qs, lim, samples, frames, sse, arrays);
    else rate_report_choice(r.j, r.qs, target, frames);
    return std::string();
}

// ---- frames a call of an RGB video (-framesPerLaunch B, else the grey path's rule on a frame's three planes of P bytes -- a
// reduced or windowed decode: the planes it writes), at most the 21 a call of picsong_encode_rgb_frames /
// picsong_decode_rgb_frames and the proxy calls takes and the frames there are
int rgb_group_frames(const Options &o, size_t P, long nframes) { return frames_per_launch(o.frames_per_launch, 3 * P, 21, nframes); }

// The frames [f0, nframes) of an RGB video (-cp 2) in groups of B through ONE call each: picsong_encode_rgb_frames on
// host-padded planes, or, -layout, picsong_encode_rgb_images on the frames as the file holds them -- one pinned staging
// area and one upload a group, one read-back of the group's 3 n streams.  Streams and _SIZE entries as frame by frame.
void encode_rgb_groups(const Options &o, picsong_ctx *ctx, hipStream_t s, int fd, size_t file_base, long f0, long nframes, StreamSink &to)
{
    const int aw = picsong_pad_dim(o.x), ah = picsong_pad_dim(o.y);
    const size_t P = (size_t)aw * ah, max_shorts = picsong_max_stream_shorts(aw, ah);
    const int B = rgb_group_frames(o, P, nframes - f0);
    const size_t raw_bytes = o.layout >= 0 ? layout_frame_bytes(o.layout, o.x, o.y) : 0;
    const size_t frame_bytes = o.layout >= 0 ? raw_bytes : 3 * P;        // a frame of the staging area
    const auto h_in = pinned_alloc<uint8_t>(frame_bytes * (size_t)B);
    const auto d_in = dev_alloc<uint8_t>(frame_bytes * (size_t)B);
    const auto h_out = pinned_alloc<uint16_t>(max_shorts * 2 * 3 * (size_t)B);
    const auto d_out = dev_alloc<uint16_t>(max_shorts * 2 * 3 * (size_t)B);
    std::vector<uint8_t> raw((size_t)o.x * o.y);
    std::vector<int> totals(3 * (size_t)B);
    for (long f = f0; f < nframes; f += B) {
        const int n = (int)std::min<long>(B, nframes - f);
        const std::string err = stage_frames(o, fd, file_base, f, n, 3, h_in, raw.data());
        if (!err.empty()) die(err);
        HIPCK(hipMemcpyAsync(d_in, h_in, frame_bytes * (size_t)n, hipMemcpyHostToDevice, s));
        if (o.layout >= 0) {
            const picsong_image im = layout_image(o.layout, d_in, o.x, o.y);
            CK(picsong_encode_rgb_images(ctx, n, &im, raw_bytes, (int)f, 7, d_out, max_shorts, s));
        } else {
            CK(picsong_encode_rgb_frames(ctx, n, d_in, d_in + P, d_in + 2 * P, 3 * P, (int)f, 7, d_out, max_shorts, s));
        }
        CK(picsong_last_totals(ctx, s, 3 * n, totals.data()));
        collect_streams(s, d_out, max_shorts, totals.data(), 3 * n, h_out, to);      // (its wait frees h_in for the next group too)
    }
}

// -searchFrames N on an RGB video (-cp 2): the -rate / -psnr / -ssim search over the first n frames through ONE call
// (search_step, RGB_FRAMES) on host-padded planes or, -layout, on the planes one picsong_ingest_frames makes of the frames
// as the file holds them.  The n frames' streams are the call's own output, written here with their _SIZE entries;
// returns the chosen qs -- the caller re-tunes the context and continues behind frame n - 1.
float rgb_search_frames(const Options &o, picsong_ctx *ctx, hipStream_t s, int fd, size_t file_base, int n, StreamSink &to)
{
    const int aw = picsong_pad_dim(o.x), ah = picsong_pad_dim(o.y);
    const size_t P = (size_t)aw * ah, max_shorts = picsong_max_stream_shorts(aw, ah);
    const size_t raw_bytes = o.layout >= 0 ? layout_frame_bytes(o.layout, o.x, o.y) : 0;
    const auto h_in = pinned_alloc<uint8_t>((o.layout >= 0 ? raw_bytes : 3 * P) * (size_t)n);
    const auto d_pad = dev_alloc<uint8_t>(3 * P * (size_t)n);
    const auto h_out = pinned_alloc<uint16_t>(max_shorts * 2 * 3 * (size_t)n);
    const auto d_out = dev_alloc<uint16_t>(max_shorts * 2 * 3 * (size_t)n);
    Dev<uint8_t> d_raw;
    if (o.layout >= 0) d_raw = dev_alloc<uint8_t>(raw_bytes * (size_t)n);
    std::vector<uint8_t> raw((size_t)o.x * o.y);
    std::string err = stage_frames(o, fd, file_base, 0, n, 3, h_in, raw.data());
    if (err.empty()) err = upload_frames(o, ctx, s, h_in, n, 3, d_raw, d_pad);
    SearchChoice r;
    if (err.empty()) err = search_step(o, ctx, s, { RGB_FRAMES, d_pad, P, n, 7 }, d_out, max_shorts, r);
    if (!err.empty()) die(err);
    collect_streams(s, d_out, max_shorts, r.totals, 3 * n, h_out, to);
    return r.qs;
}

// ---- RGB coding (CodingEngine::runImage / runVideo, RGB branches: CodingEngine.cu:598-633,676-712,
// 760-818,873-930): the input holds planar R, G, B planes per frame; RCT / ICT with the level shift
// fused, then every component is coded as a frame of its own with its own LUT and appended to <o>,
// its length to <o>_SIZE.  Header: image -> component 0 only (iter = component), video -> all three
// components of frame 0 (iter = frame).
int run_encode_rgb(const Options &o, size_t file_base, long nframes)
{
    HIPCK(hipSetDevice(o.device));
    const int aw = picsong_pad_dim(o.x), ah = picsong_pad_dim(o.y);
    const size_t P = (size_t)aw * ah, max_shorts = picsong_max_stream_shorts(aw, ah);
    picsong_params params = make_params(o);
    Ctx ctx;
    CK(picsong_ctx_create(&params, o.device, &ctx.p));
    load_lut(ctx, o, o.wl, 3, o.k, o.cp);
    const Stream s = stream_create();
    // a frame's three padded planes, back to back pinned and on the device; -layout: the frame of the file as it is,
    // pinned and on the device, where the planes are then made
    const size_t raw_bytes = o.layout >= 0 ? layout_frame_bytes(o.layout, o.x, o.y) : 0;
    const auto h_in = pinned_alloc<uint8_t>(std::max(raw_bytes, 3 * P));
    const auto d_in = dev_alloc<uint8_t>(3 * P);
    Dev<uint8_t> d_raw;
    if (o.layout >= 0) d_raw = dev_alloc<uint8_t>(raw_bytes);
    Dev<char> d_c[3];
    for (int c = 0; c < 3; c++) d_c[c] = dev_alloc<char>(P * 4);
    // the three components of a frame through ONE launch per stage (picsong_encode_rgb_frame) wherever the library
    // offers it: -cp 2; otherwise plane by plane
    const bool batched = o.cp != 3;
    const auto h_out = pinned_alloc<uint16_t>(max_shorts * 2 * (batched ? 3 : 1));
    const auto d_out = dev_alloc<uint16_t>(max_shorts * 2 * (batched ? 3 : 1));
    std::vector<uint8_t> raw((size_t)o.x * o.y);
    const int fd = open(o.input.c_str(), O_RDONLY);
    if (fd < 0) die("Cannot open input file " + o.input);
    StreamSink to(o.output);
    auto t0 = std::chrono::steady_clock::now();
    // a video (-cp 2): groups of frames through one call each (encode_rgb_groups) -- behind the first frame where that one
    // carries the -rate / -psnr search; an image and -cp 3: frame by frame, here
    const bool grouped = o.video && batched;
    long nloop = grouped ? ((o.has_rate || o.has_quality()) ? 1 : 0) : nframes;
    long searched = 0;                                   // -searchFrames: the frames the n-frame search call coded itself
    if (grouped && o.search_frames > 0) {
        searched = std::min<long>(o.search_frames, nframes);
        CK(picsong_ctx_set_qs(ctx, rgb_search_frames(o, ctx, s, fd, file_base, (int)searched, to)));
        nloop = 0;
    }
    for (long f = 0; f < nloop; f++) {
        const std::string short_input = stage_frames(o, fd, file_base, f, 1, 3, h_in, raw.data());
        if (!short_input.empty()) die(short_input);
        if (o.layout >= 0) {
            HIPCK(hipMemcpyAsync(d_raw, h_in, raw_bytes, hipMemcpyHostToDevice, s));
            const picsong_image im = layout_image(o.layout, d_raw, o.x, o.y);
            CK(picsong_ingest_frames(ctx, 1, &im, 0, d_in, 0, s));
        } else {
            HIPCK(hipMemcpyAsync(d_in, h_in, 3 * P, hipMemcpyHostToDevice, s));
        }
        HIPCK(hipStreamSynchronize(s));                  // h_in is reused for the next frame
        int totals[3] = { 0, 0, 0 };
        if ((o.has_rate || o.has_quality()) && f == 0) {
            // the search on the first frame (an image: the frame); the rest of a video is coded at the result
            SearchChoice r;
            const std::string err = search_step(o, ctx, s, { RGB_FRAME, d_in, P, 1, o.video ? 7 : 1 }, d_out, max_shorts, r);
            if (!err.empty()) die(err);
            CK(picsong_ctx_set_qs(ctx, r.qs));
            std::copy(r.totals, r.totals + 3, totals);
        } else if (batched) {
            CK(picsong_encode_rgb_frame(ctx, d_in, d_in + P, d_in + 2 * P, o.video ? (f == 0 ? 7 : 0) : 1, d_out, max_shorts, s));
            CK(picsong_last_totals(ctx, s, 3, totals));
        } else {
            CK(picsong_rgb_forward(ctx, d_in, d_in + P, d_in + 2 * P, d_c[0], d_c[1], d_c[2], s));
        }
        if (batched) collect_streams(s, d_out, max_shorts, totals, 3, h_out, to);
        for (int c = 0; c < 3 && !batched; c++) {
            CK(picsong_encode_plane(ctx, d_c[c], c, o.video ? (f == 0) : (c == 0), d_out, s));
            CK(picsong_last_total(ctx, s, &totals[c]));
            collect_streams(s, d_out, 0, &totals[c], 1, h_out, to);
        }
    }
    if (grouped && std::max(nloop, searched) < nframes) encode_rgb_groups(o, ctx, s, fd, file_base, std::max(nloop, searched), nframes, to);
    close(fd);
    double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::cout << "The time spent with the app without considering allocation periods is: " << sec << std::endl;
    if (o.has_rate) rate_report_achieved(o, to.total_shorts, nframes);
    write_metrics(o, "encode_rgb", nframes, sec, 0, 0, 0, to.total_shorts);
    return 0;
}

// ---- training (-train <outFolder>): the input read exactly as an encode reads it, its frames through the training
// calls in groups of B per launch (grey) or a frame at a time (RGB: one launch per stage, component c into slot c),
// then the counts of every component made into a table (picsong_lut_from_counts) and written as the folder's files:
// R for a grey input -- what a grey encode loads -- and R, G, B for an RGB one.
int run_train(const Options &o, size_t file_base, long nframes)
{
    HIPCK(hipSetDevice(o.device));
    const int aw = picsong_pad_dim(o.x), ah = picsong_pad_dim(o.y), comps = o.is_rgb ? 3 : 1;
    const size_t P = (size_t)aw * ah;
    picsong_params params = make_params(o);
    Ctx ctx;
    CK(picsong_ctx_create(&params, o.device, &ctx.p));
    // the geometry counted for: the prior folder's, or the shipped folders' 15 / 3 / 1 / 4 / 9 / 7
    picsong_lut_info geo;
    memset(&geo, 0, sizeof geo);
    geo.n_bitplanes = 15; geo.n_subbands = 3; geo.ctx_ref = 1; geo.ctx_sign = 4; geo.ctx_sig = 9; geo.precision = 7;
    std::vector<std::vector<int32_t>> prior((size_t)comps);
    if (!o.lut_folder.empty()) {
        for (int c = 0; c < comps; c++) {
            picsong_lut_info pi;
            CK(picsong_lut_load(o.lut_folder.c_str(), c + 1, o.wl, o.lut_fill, &pi, nullptr, 0));
            prior[(size_t)c].resize((size_t)pi.n_ref + pi.n_sig + pi.n_sign);
            CK(picsong_lut_load(o.lut_folder.c_str(), c + 1, o.wl, o.lut_fill, &pi, prior[(size_t)c].data(), prior[(size_t)c].size()));
            if (c == 0) geo = pi;
        }
    }
    CK(picsong_train_begin(ctx, &geo));
    picsong_lut_info info;
    CK(picsong_train_info(ctx, &info));
    const long planes = nframes * comps;
    const int B = o.is_rgb ? 3 : frames_per_launch(o.frames_per_launch, P, 16, planes);      // (RGB: the three planes of a frame)
    const Stream s = stream_create();
    const auto h_in = pinned_alloc<uint8_t>(P * B);
    const auto d_in = dev_alloc<uint8_t>(P * B);
    std::vector<uint8_t> raw((size_t)o.x * o.y);
    const int fd = open(o.input.c_str(), O_RDONLY);
    if (fd < 0) die("Cannot open input file " + o.input);
    auto t0 = std::chrono::steady_clock::now();
    for (long f = 0; f < planes; f += B) {
        const int n = (int)std::min<long>(B, planes - f);
        const std::string err = stage_frames(o, fd, file_base, f, n, 1, h_in, raw.data());      // (-layout is refused with -train)
        if (!err.empty()) die(err);
        HIPCK(hipMemcpyAsync(d_in, h_in, P * n, hipMemcpyHostToDevice, s));
        if (o.is_rgb) CK(picsong_train_rgb_frame(ctx, d_in, d_in + P, d_in + 2 * P, s));
        else CK(picsong_train_frames(ctx, n, d_in, P, s));
        HIPCK(hipStreamSynchronize(s));                      // h_in and d_in are reused for the next group
    }
    const int entries = picsong_train_counts(ctx, 0, s, nullptr, 0);
    if (entries <= 0) die(std::string("picsong_train_counts failed: ") + picsong_last_error());
    std::vector<uint64_t> counts((size_t)entries * 2);
    std::vector<int32_t> table((size_t)entries);
    unsigned long long symbols = 0;
    long seen = 0;
    for (int c = 0; c < comps; c++) {
        CK(picsong_train_counts(ctx, c, s, counts.data(), (size_t)entries));
        for (int e = 0; e < entries; e++) {
            const uint64_t t = counts[2 * (size_t)e] + counts[2 * (size_t)e + 1];
            symbols += t;
            seen += t != 0;
        }
        const bool has_prior = prior[(size_t)c].size() >= (size_t)entries;
        CK(picsong_lut_from_counts(&info, counts.data(), has_prior ? prior[(size_t)c].data() : nullptr, table.data()));
        CK(picsong_lut_save(o.train.c_str(), c + 1, &info, o.wl, table.data()));
    }
    int flag = 0;
    CK(picsong_range_flag(ctx, s, &flag));
    double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::cout << "Trained " << o.train << " for -wl " << o.wl << ": " << symbols << " symbols counted, " << seen << " of "
              << (long)entries * comps << " entries seen" << std::endl;
    if (flag) std::cout << "Warning: codeblocks with more than 16 bit-planes were left out." << std::endl;
    std::cout << "The time spent with the app without considering allocation periods is: " << sec << std::endl;
    write_metrics(o, "train", nframes, sec, 0, 0, 0, 0);
    CK(picsong_train_end(ctx));
    close(fd);
    return 0;
}

constexpr long kProfFrames = 256;     // frames per pipeline slot whose stages are timed with HIP events

// ---- -bps 9..16: ONE grey still image of 16-bit samples, coded (picsong_encode_images, GREY16) and decoded
// (picsong_decode_images); or, -isRGB 1 -components 3, one RGB still image or a video of 16-bit samples, coded
// (picsong_encode_rgb_images) and decoded (picsong_decode_rgb_images) straight-line, a group of frames a call.  What every
// other mode says when it meets such a depth:
const char *const kDeepBuilt =
    "With -bps 9..16 this build codes one grey still image (-cd 0: a raw file of W*H little-endian 16-bit samples or a P5 PGM with "
    "maxval > 255) and decodes it (-cd 1, -drop allowed); with -isRGB 1 -components 3 it codes one RGB still image or a video (-video 1 "
    "-frames F, -framesPerLaunch 1..21) from a raw file of little-endian 16-bit samples -- -layout planar (the default: R, G, B planes "
    "of W*H samples a frame), rgb (6 bytes a pixel) or rgba (8 bytes a pixel) -- and decodes it to such a file (-drop allowed): not a "
    "grey -video, -rate, -psnr, -ssim, -train, -reduce, -window, -gpus, -cp 3, -compare, a PGM for RGB, -layout grey with RGB, bgr or bgra, "
    "or a colour -layout without -isRGB; -signedOrUnsigned 1 is not built.";
void deep_check_mode(const Options &o, bool rgb, int bps)
{
    if (bps < 9 || bps > 16 || o.signed_or_unsigned != 0) die(std::string("Only unsigned samples of 8..16 bits are built. ") + kDeepBuilt);
    if (o.has_rate || o.has_quality() || !o.train.empty() || o.reduce > 0 || o.win || o.gpus > 1 || !o.devices.empty() || !o.compare.empty() ||
        o.search_frames > 0)
        die(kDeepBuilt);
    if (!rgb && (o.video || o.layout > PICSONG_LAYOUT_GREY8)) die(kDeepBuilt);
    if (rgb && (o.layout == PICSONG_LAYOUT_GREY8 || o.layout == PICSONG_LAYOUT_BGR24 || o.layout == PICSONG_LAYOUT_BGRA32)) die(kDeepBuilt);
}
// the 16-bit layout of a deep RGB file (-layout planar | rgb | rgba, default planar), its bytes a frame and its picsong_image
int deep_rgb_layout(int layout) { return layout == PICSONG_LAYOUT_RGB24 ? PICSONG_LAYOUT_RGB48 : (layout == PICSONG_LAYOUT_RGBA32 ? PICSONG_LAYOUT_RGBA64 : PICSONG_LAYOUT_PLANAR3_16); }
size_t deep_rgb_frame_bytes(int layout16, int w, int h) { return (size_t)w * (size_t)h * (layout16 == PICSONG_LAYOUT_RGBA64 ? 8u : 6u); }
picsong_image deep_rgb_image(int layout16, void *d, int w, int h)
{
    picsong_image im;
    im.data = d; im.layout = layout16; im.plane_stride = (size_t)w * (size_t)h * 2;
    im.pitch = (size_t)w * (layout16 == PICSONG_LAYOUT_PLANAR3_16 ? 2u : (layout16 == PICSONG_LAYOUT_RGB48 ? 6u : 8u));
    return im;
}
// -bps 9..16 -isRGB 1 -components 3: the frames as the raw file holds them, a group of B a call of picsong_encode_rgb_images;
// streams and _SIZE entries as the 8-bit RGB paths write them (an image: the header on component 0; a video: on frame 0's three)
int run_encode_deep_rgb(const Options &o, const Pgm &pgm)
{
    if (pgm.is_pgm) die(std::string("A PGM holds one component. ") + kDeepBuilt);
    const long nframes = o.video ? o.frames : 1;
    if (nframes <= 0) die("Incorrect parameters. Please choose valid values. (-frames)");
    if (o.frames_per_launch > 21) die(std::string("Incorrect parameters. -framesPerLaunch takes 1..21 RGB frames. ") + kDeepBuilt);
    const int layout16 = deep_rgb_layout(o.layout);
    const size_t fb = deep_rgb_frame_bytes(layout16, o.x, o.y);
    {   // (before anything is created: a file of another kind, a grey one for instance, is too short)
        std::ifstream in(o.input, std::ios::binary | std::ios::ate);
        if (!in) die("Cannot open input file " + o.input);
        if ((size_t)in.tellg() < fb * (size_t)nframes) die(std::string(kShortInput) + " " + kDeepBuilt);
    }
    HIPCK(hipSetDevice(o.device));
    picsong_params p = make_params(o);
    p.frames = o.video ? (int)nframes : 0;
    Ctx ctx;
    CK(picsong_ctx_create(&p, o.device, &ctx.p));
    load_lut(ctx, o, o.wl, 3, o.k, o.cp);
    int aw, ah, ncb;
    CK(picsong_ctx_padded_dims(ctx, &aw, &ah, &ncb));
    const size_t max_shorts = picsong_max_stream_shorts(aw, ah);
    const int B = frames_per_launch(o.frames_per_launch, 6 * (size_t)aw * ah, 21, nframes);
    const Stream s = stream_create();
    const auto h_in = pinned_alloc<uint8_t>(fb * (size_t)B);
    const auto d_in = dev_alloc<uint8_t>(fb * (size_t)B);
    const auto h_out = pinned_alloc<uint16_t>(max_shorts * 2 * 3 * (size_t)B);
    const auto d_out = dev_alloc<uint16_t>(max_shorts * 2 * 3 * (size_t)B);
    std::vector<int> totals(3 * (size_t)B);
    const int fd = open(o.input.c_str(), O_RDONLY);
    if (fd < 0) die("Cannot open input file " + o.input);
    { std::ofstream t0(o.output, std::ios::binary | std::ios::trunc), t1(o.output + "_SIZE", std::ios::trunc); }
    StreamSink to(o.output);
    auto t0 = std::chrono::steady_clock::now();
    for (long f = 0; f < nframes; f += B) {
        const int n = (int)std::min<long>(B, nframes - f);
        if (!pread_exact(fd, h_in, fb * (size_t)n, (size_t)f * fb)) die(kShortInput);
        HIPCK(hipMemcpyAsync(d_in, h_in, fb * (size_t)n, hipMemcpyHostToDevice, s));
        const picsong_image im = deep_rgb_image(layout16, d_in, o.x, o.y);
        CK(picsong_encode_rgb_images(ctx, n, &im, fb, (int)f, o.video ? 7 : 1, d_out, max_shorts, s));
        CK(picsong_last_totals(ctx, s, 3 * n, totals.data()));
        int flag = 0;
        CK(picsong_range_flag(ctx, s, &flag));
        if (flag) {
            to.out.close();
            std::remove(o.output.c_str());
            std::remove((o.output + "_SIZE").c_str());
            die("A coefficient of this input reaches 2^15, beyond what the coder codes (picsong_depth_range_guaranteed_rgb says which "
                "depths never do): nothing written.");
        }
        collect_streams(s, d_out, max_shorts, totals.data(), 3 * n, h_out, to);
    }
    close(fd);
    double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::cout << "The time spent with the app without considering allocation periods is: " << sec << std::endl;
    write_metrics(o, "encode_rgb", nframes, sec, 0, 0, 0, to.total_shorts);
    return 0;
}
int run_encode_deep(const Options &o, const Pgm &pgm)
{
    deep_check_mode(o, o.is_rgb != 0, o.bps);
    if (o.cp == 3) die(std::string("-cp 3 is not built for -bps 9..16. ") + kDeepBuilt);
    if (o.is_rgb) return run_encode_deep_rgb(o, pgm);
    if (pgm.is_pgm && pgm.maxval <= 255) die("Incorrect parameters. -bps " + std::to_string(o.bps) + " takes a P5 PGM with maxval > 255 (two bytes a sample).");
    const size_t n = (size_t)o.x * (size_t)o.y;
    std::vector<uint16_t> img(n);
    {
        std::ifstream in(o.input, std::ios::binary);
        if (!in) die("Cannot open input file " + o.input);
        if (!read_exact(in, img.data(), n * 2, pgm.is_pgm ? pgm.offset : 0)) die(kShortInput);
        // (Netpbm: a PGM's two-byte samples are big-endian; a raw file's are little-endian, the host's order)
        if (pgm.is_pgm) for (uint16_t &v : img) v = (uint16_t)((v >> 8) | (v << 8));
    }
    HIPCK(hipSetDevice(o.device));
    picsong_params p = make_params(o);
    p.frames = 0;
    Ctx ctx;
    CK(picsong_ctx_create(&p, o.device, &ctx.p));
    load_lut(ctx, o, o.wl, 1, o.k, o.cp);
    int aw, ah, ncb;
    CK(picsong_ctx_padded_dims(ctx, &aw, &ah, &ncb));
    const size_t max_shorts = picsong_max_stream_shorts(aw, ah);
    const Stream s = stream_create();
    const auto d_raw = dev_alloc<uint16_t>(n * 2);
    const auto d_out = dev_alloc<uint16_t>(max_shorts * 2);
    std::vector<uint16_t> out(max_shorts);
    auto t0 = std::chrono::steady_clock::now();
    HIPCK(hipMemcpyAsync(d_raw, img.data(), n * 2, hipMemcpyHostToDevice, s));
    picsong_image im;
    im.data = d_raw; im.pitch = (size_t)o.x * 2; im.plane_stride = 0; im.layout = PICSONG_LAYOUT_GREY16;
    CK(picsong_encode_images(ctx, 1, &im, 0, 0, d_out, max_shorts, s));
    int total = 0, flag = 0;
    CK(picsong_last_totals(ctx, s, 1, &total));
    HIPCK(hipMemcpyAsync(out.data(), d_out, (size_t)total * 2, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    CK(picsong_range_flag(ctx, s, &flag));
    double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (flag) die("A coefficient of this image reaches 2^15, beyond what the coder codes (picsong_depth_range_guaranteed says which "
                  "depths never do): nothing written.");
    {
        std::ofstream f(o.output, std::ios::binary | std::ios::trunc);
        if (!f) die("Cannot open output file " + o.output);
        f.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)((size_t)total * 2));
    }
    std::cout << "The time spent with the app without considering allocation periods is: " << sec << std::endl;
    write_metrics(o, "encode", 1, sec, 0, 0, 0, total);
    return 0;
}

// ---- what -rate, -psnr and -ssim refuse alike, in this order; with_rate / with_psnr: that flag is given too and wins
void check_search_flag(const Options &o, const std::string &flag, bool with_rate, bool with_psnr)
{
    const std::string pre = "Incorrect parameters. " + flag;
    if (o.has_qs) die(pre + " chooses the quantiser: it cannot be combined with -qs.");
    if (with_rate) die(pre + " cannot be combined with -rate.");
    if (with_psnr) die(pre + " cannot be combined with -psnr.");
    if (o.type != 1) die(pre + " applies to lossy coding (-type 1) only.");
    if (o.cp == 3) die(pre + " does not apply to -cp 3.");
    if (!o.train.empty()) die(pre + " does not apply to -train.");
}

// ---- coding engine: CodingEngine::runImage / runVideo call sequence ---------------------------
int run_encode(Options o)
{
    Pgm pgm = sniff_pgm(o.input);
    if (pgm.is_pgm) {
        if (o.x <= 0) o.x = pgm.w;
        if (o.y <= 0) o.y = pgm.h;
        if (o.x != pgm.w || o.y != pgm.h) die("Incorrect parameters. -xSize/-ySize differ from the PGM header.");
    }
    // Launcher.cu:132
    if (o.qs < 0 || o.qs > 1 || o.wl < 1 || o.x <= 0 || o.y <= 0 || o.wl > 10 || o.input.empty() || (o.output.empty() && o.train.empty()) ||
        o.cb_width % 64 != 0 || o.cb_height > 20 || o.cb_height < 18 || o.cp < 2 || o.cp > 3 || o.k < 0 || o.k > 65.535f)
        die("Incorrect parameters. Please choose valid values.");
    if (!((o.is_rgb && o.components == 3) || (!o.is_rgb && o.components == 1)))
        die("Incorrect parameters. Use -components 1, or -isRGB 1 -components 3 (planar R,G,B planes).");
    if (o.cp == 3 && o.k > 0) die("Incorrect parameters. -cp 3 has no complexity-scalable mode (-k must be 0).");
    if (o.signed_or_unsigned != 0 || o.bps != 8) return run_encode_deep(o, pgm);
    const long nframes = o.video ? o.frames : 1;
    if (nframes <= 0) die("Incorrect parameters. Please choose valid values. (-frames)");
    if (o.has_rate) check_search_flag(o, "-rate", false, false);
    if (o.has_psnr) check_search_flag(o, "-psnr", o.has_rate, false);
    if (o.has_ssim) {
        check_search_flag(o, "-ssim", o.has_rate, o.has_psnr);
        if (o.x < 8 || o.y < 8) die("Incorrect parameters. -ssim needs a frame of 8 x 8 samples or more.");
    }
    if (o.search_frames > 0) {
        if (!o.video) die("Incorrect parameters. -searchFrames applies to a video (-video 1) only.");
        if (!o.has_rate && !o.has_quality()) die("Incorrect parameters. -searchFrames needs -rate or -psnr (or -ssim): it sizes their search.");
        if (o.search_frames > (o.is_rgb ? 21 : 16))
            die(o.is_rgb ? "Incorrect parameters. -searchFrames takes 1..21 frames of an RGB video." : "Incorrect parameters. -searchFrames takes 1..16 grey frames.");
    }
    layout_check_context(o.layout, o.is_rgb != 0);
    if (o.layout >= 0 && !o.train.empty()) die("Incorrect parameters. -layout does not apply to -train.");
    if (!o.train.empty()) {
        if (o.k > 0) die("Incorrect parameters. -train counts the two-pass coder's decisions (-k must be 0).");
        if (o.cp == 3) die("Incorrect parameters. -train does not apply to -cp 3.");
        return run_train(o, pgm.is_pgm ? pgm.offset : 0, nframes);
    }
    if (o.is_rgb) return run_encode_rgb(o, pgm.is_pgm ? pgm.offset : 0, nframes);
    // ---- devices: -gpus N takes devices D .. D+N-1, --devices names them (a device may repeat: several
    // worker sets on one GPU, which is also how the sharded path is exercised on a one-GPU box)
    std::vector<int> devs;
    {
        int ndev = 0;
        HIPCK(hipGetDeviceCount(&ndev));
        if (!o.devices.empty()) {
            std::stringstream ss(o.devices);
            std::string tok;
            while (std::getline(ss, tok, ',')) if (!tok.empty()) devs.push_back(std::stoi(tok));
        } else {
            for (int i = 0; i < (o.gpus < 1 ? 1 : o.gpus); i++) devs.push_back(o.device + i);
        }
        if (devs.empty()) die("Incorrect parameters. Please choose valid values. (--devices)");
        for (int d : devs)
            if (d < 0 || d >= ndev) die("Incorrect parameters. -gpus / --devices name GPU " + std::to_string(d) + ", this node has " + std::to_string(ndev));
        if (!o.video && devs.size() > 1) devs.resize(1);           // one image = one frame = one GPU
    }
    const int ndevs = (int)devs.size();
    const int aw = picsong_pad_dim(o.x), ah = picsong_pad_dim(o.y);
    const size_t P = (size_t)aw * ah, max_shorts = picsong_max_stream_shorts(aw, ah);
    const int B = (!o.video || o.cp == 3) ? 1 : frames_per_launch(o.frames_per_launch, P, 16, nframes);
    const long ngroups = (nframes + B - 1) / B;
    // slots of the pipeline: at least 6 for a video (2 readers | launch | run | collect | 2 writers overlap),
    // a multiple of the device count so that slot i always belongs to device i mod ndevs
    int nstreams = o.video ? ((o.streams < 3 ? 3 : o.streams) + 3) : 1;
    if (o.video) nstreams = (nstreams + ndevs - 1) / ndevs * ndevs;
    if (nstreams < ndevs) nstreams = ndevs;

    const size_t frame_bytes = (size_t)o.x * o.y, file_base = pgm.is_pgm ? pgm.offset : 0;
    picsong_params params = make_params(o);
    std::vector<Worker> w((size_t)nstreams);
    for (int i = 0; i < nstreams; i++) {
        Worker &k = w[(size_t)i];
        k.device = devs[(size_t)(i % ndevs)];
        HIPCK(hipSetDevice(k.device));
        CK(picsong_ctx_create(&params, k.device, &k.ctx.p));
        if (nstreams > 1) CK(picsong_ctx_set_pipelined(k.ctx, 1));     // the video engine keeps frames in flight
        load_lut(k.ctx, o, o.wl, 1, o.k, o.cp);
        k.stream = stream_create();
        k.h_in = pinned_alloc<uint8_t>(P * B);
        k.d_in = dev_alloc<uint8_t>(P * B);
        k.h_out = pinned_alloc<uint16_t>(max_shorts * 2 * B);
        k.d_out = dev_alloc<uint16_t>(max_shorts * 2 * B);
        k.h_raw.resize(frame_bytes);
        if (o.layout >= 0) k.d_raw = dev_alloc<uint8_t>(frame_bytes * (size_t)B);
        // stage timers (HIP events): at most kProfFrames launches per slot are timed, so the event count does
        // not grow with the video; "BPC acum time" scales their mean to all frames
        CK(picsong_profile_begin(k.ctx, (int)std::min<long>((ngroups + nstreams - 1) / nstreams, kProfFrames)));
    }
    const int fd = open(o.input.c_str(), O_RDONLY);
    if (fd < 0) die("Cannot open input file " + o.input);
    if ((o.has_rate || o.has_quality()) && o.video) {
        // -rate on a video: the first slot's context (rank 0 of -gpus N) searches on the first min(frames, 16) frames and
        // their summed target, then every context takes the chosen qs: the stream has one header, hence one qs
        const int n = (int)std::min<long>(nframes, o.search_frames > 0 ? o.search_frames : 16);
        Worker &k = w[0];
        HIPCK(hipSetDevice(k.device));
        const auto h_f = pinned_alloc<uint8_t>(P * (size_t)n);
        const auto d_f = dev_alloc<uint8_t>(P * (size_t)n);
        const auto d_s = dev_alloc<uint16_t>(max_shorts * 2 * (size_t)n);
        Dev<uint8_t> d_r;               // -layout: the frames as read, padded on the device
        if (o.layout >= 0) d_r = dev_alloc<uint8_t>(frame_bytes * (size_t)n);
        std::string err = stage_frames(o, fd, file_base, 0, n, 1, h_f, k.h_raw.data());
        if (err.empty()) err = upload_frames(o, k.ctx, k.stream, h_f, n, 1, d_r, d_f);
        SearchChoice r;                 // the target, or the limit, over all n frames
        if (err.empty()) err = search_step(o, k.ctx, k.stream, { GREY_FRAMES, d_f, P, n, 0 }, d_s, max_shorts, r);
        if (!err.empty()) die(err);
        for (auto &x : w) CK(picsong_ctx_set_qs(x.ctx, r.qs));
    }
    // image: one truncating write (IOManager.ipp:615-620); video: append + _SIZE (:176-190)
    const int ofd = open(o.output.c_str(), O_WRONLY | O_CREAT | (o.video ? 0 : O_TRUNC), 0644);
    if (ofd < 0) die("Cannot open output file " + o.output);
    const off_t out_base = o.video ? lseek(ofd, 0, SEEK_END) : 0;
    long total_shorts = 0;
    std::vector<int> frame_totals((size_t)nframes, 0);
    auto t0 = std::chrono::steady_clock::now();

    // slot state machine: FREE -(reader)-> FILLED -(main)-> LAUNCHED -(collector)-> COLLECTED
    // -(writer)-> FREE; a slot carries one GROUP of up to B consecutive frames; `expect` is the group the
    // slot takes next, so groups g and g + S never race
    enum { FREE = 0, FILLED = 1, LAUNCHED = 2, COLLECTED = 3 };
    struct SlotState { int state = FREE; long expect = 0; int n = 0; off_t offset[16]; int total[16]; };
    std::vector<SlotState> st((size_t)nstreams);
    for (int i = 0; i < nstreams; i++) st[(size_t)i].expect = i;
    auto group_frames = [&](long g) { return (int)std::min<long>(B, nframes - g * B); };
    std::mutex mu;
    std::condition_variable cv;
    std::string failure;                      // first error of a helper thread (reported by main)
    // where the host threads spend their time (reported with --metrics)
    std::vector<double> t_read(16, 0.0);
    double t_wait_gpu = 0.0, t_write = 0.0, t_main_wait = 0.0, t_launch = 0.0;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double>(b - a).count(); };

    auto reader = [&](int r, int nreaders) {
        for (long g = r; g < ngroups; g += nreaders) {
            const size_t si = (size_t)(g % nstreams);
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !failure.empty() || (st[si].state == FREE && st[si].expect == g); });
                if (!failure.empty()) return;
            }
            Worker &k = w[si];
            const int n = group_frames(g);
            const auto tr0 = now();
            const std::string err = stage_frames(o, fd, file_base, g * B, n, 1, k.h_in, k.h_raw.data());
            t_read[(size_t)r] += secs(tr0, now());
            std::lock_guard<std::mutex> lk(mu);
            if (!err.empty() && failure.empty()) failure = err;
            st[si].n = n;
            st[si].state = FILLED;
            cv.notify_all();
        }
    };
    // collector (one thread, group order): waits for the group's lengths and fixes every frame's place in
    // the file; writers (any order): copy the codestreams back over the slot's device's own host link,
    // pwrite them there and free the slot
    auto collector = [&] {
        off_t offset = out_base;
        for (long g = 0; g < ngroups; g++) {
            const size_t si = (size_t)(g % nstreams);
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !failure.empty() || (st[si].state == LAUNCHED && st[si].expect == g); });
                if (!failure.empty()) return;
            }
            Worker &k = w[si];
            (void)hipSetDevice(k.device);
            const int n = st[si].n;
            int totals[16] = { 0 };
            std::string err;
            const auto tw0 = now();
            if (B == 1) { if (picsong_last_total(k.ctx, k.stream, &totals[0]) != PICSONG_OK) err = picsong_last_error(); }
            else if (picsong_last_totals(k.ctx, k.stream, n, totals) != PICSONG_OK) err = picsong_last_error();
            t_wait_gpu += secs(tw0, now());
            std::lock_guard<std::mutex> lk(mu);
            if (!err.empty() && failure.empty()) failure = err;
            for (int j = 0; j < n; j++) {
                frame_totals[(size_t)(g * B + j)] = totals[j];
                total_shorts += totals[j];
                st[si].offset[j] = offset;
                st[si].total[j] = totals[j];
                offset += (off_t)totals[j] * 2;
            }
            st[si].state = COLLECTED;
            cv.notify_all();
        }
    };
    std::vector<double> t_write_v(8, 0.0);
    auto writer = [&](int r, int nwriters) {
        for (long g = r; g < ngroups; g += nwriters) {
            const size_t si = (size_t)(g % nstreams);
            SlotState ss;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !failure.empty() || (st[si].state == COLLECTED && st[si].expect == g); });
                if (!failure.empty()) return;
                ss = st[si];
            }
            const auto tw1 = now();
            std::string err;
            (void)hipSetDevice(w[si].device);
            for (int j = 0; j < ss.n && err.empty(); j++)
                if (hipMemcpyAsync(w[si].h_out + (size_t)j * max_shorts, w[si].d_out + (size_t)j * max_shorts,
                                   (size_t)ss.total[j] * 2, hipMemcpyDeviceToHost, w[si].stream) != hipSuccess)
                    err = "HIP error while copying a codestream back";
            if (err.empty() && hipStreamSynchronize(w[si].stream) != hipSuccess) err = "HIP error while copying a codestream back";
            for (int j = 0; j < ss.n && err.empty(); j++)
                if (!pwrite_exact(ofd, w[si].h_out + (size_t)j * max_shorts, (size_t)ss.total[j] * 2, (size_t)ss.offset[j]))
                    err = "Cannot write the output file " + o.output;
            t_write_v[(size_t)r] += secs(tw1, now());
            std::lock_guard<std::mutex> lk(mu);
            if (!err.empty() && failure.empty()) failure = err;
            st[si].state = FREE;
            st[si].expect = g + nstreams;
            cv.notify_all();
        }
    };
    int nreaders = ngroups > 1 ? 2 : 1;
    if (const char *e = getenv("PICSONG_READERS")) { int v = atoi(e); if (v >= 1 && v <= 16) nreaders = v; }
    if (nreaders > nstreams - 1 && nstreams > 1) nreaders = nstreams - 1;
    std::vector<std::thread> threads;
    for (int r = 0; r < nreaders; r++) threads.emplace_back(reader, r, nreaders);
    int nwriters = ngroups > 1 ? 2 : 1;
    if (const char *e = getenv("PICSONG_WRITERS")) { int v = atoi(e); if (v >= 1 && v <= 8) nwriters = v; }
    threads.emplace_back(collector);
    for (int r = 0; r < nwriters; r++) threads.emplace_back(writer, r, nwriters);
    for (long g = 0; g < ngroups; g++) {
        const size_t si = (size_t)(g % nstreams);
        const auto tm0 = now();
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !failure.empty() || (st[si].state == FILLED && st[si].expect == g); });
            if (!failure.empty()) break;
        }
        const auto tm1 = now();
        t_main_wait += secs(tm0, tm1);
        Worker &k = w[si];
        const int n = st[si].n;
        std::string err;
        if (hipSetDevice(k.device) != hipSuccess) err = "HIP error in the frame upload";
        else if (!(err = upload_frames(o, k.ctx, k.stream, k.h_in, n, 1, k.d_raw, k.d_in)).empty()) { }
        else if ((o.has_rate || o.has_quality()) && !o.video) {
            // an image: one search call (synchronous); its length is the context's last total, as after picsong_encode_frame
            SearchChoice r;
            err = search_step(o, k.ctx, k.stream, { GREY_FRAME, k.d_in, 0, 1, 0 }, k.d_out, 0, r);
        }
        else if (B == 1) { if (picsong_encode_frame(k.ctx, k.d_in, g == 0 ? 0 : 1, k.d_out, k.stream) != PICSONG_OK) err = picsong_last_error(); }
        else if (picsong_encode_frames(k.ctx, n, k.d_in, P, (int)(g * B), k.d_out, max_shorts, k.stream) != PICSONG_OK) err = picsong_last_error();
        t_launch += secs(tm1, now());
        std::lock_guard<std::mutex> lk(mu);
        if (!err.empty() && failure.empty()) failure = err;
        st[si].state = LAUNCHED;
        cv.notify_all();
    }
    for (auto &t : threads) t.join();
    close(fd);
    close(ofd);
    if (!failure.empty()) die(failure);
    if (o.video) SizeList(o.output + "_SIZE").append(frame_totals.data(), (size_t)nframes);      // in frame order
    for (double v : t_write_v) t_write += v;
    double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!o.metrics.empty()) {
        double rd = 0; for (double v : t_read) rd += v;
        std::cout << "host pipeline seconds: read(sum of " << nreaders << " readers) " << rd << ", main waiting for frames "
                  << t_main_wait << ", main launching " << t_launch << ", writer waiting for the GPU " << t_wait_gpu
                  << ", writer writing " << t_write << "; " << ndevs << " device(s), " << B << " frame(s) per launch" << std::endl;
    }

    double dwt = 0, bpc = 0, pack = 0;
    long counted = 0;
    for (auto &k : w) {
        int n = 0;
        std::vector<float> ms(3 * (size_t)std::min<long>((ngroups + nstreams - 1) / nstreams, kProfFrames) + 3);
        (void)hipSetDevice(k.device);
        CK(picsong_profile_read(k.ctx, &n, ms.data(), (int)(ms.size() / 3)));
        for (int i = 0; i < n; i++) { dwt += ms[3 * i]; bpc += ms[3 * i + 1]; pack += ms[3 * i + 2]; counted++; }
    }
    std::cout << "The time spent with the app without considering allocation periods is: " << sec << std::endl;
    std::cout << "BPC acum time is: " << (counted ? bpc / counted * (double)ngroups : 0.0) / 1e3 << std::endl;
    if (o.has_rate) rate_report_achieved(o, total_shorts, nframes);
    write_metrics(o, "encode", nframes, sec, counted ? dwt / counted / B : 0, counted ? bpc / counted / B : 0,
                  counted ? pack / counted / B : 0, total_shorts);
    return 0;
}

// A decode context from a stream's header.  picsong_ctx_create keeps the coding launcher's -qs range (0, 1]; a stream coded
// by -rate may carry any gain the header stores (up to 1.6383): such a context is created at 1 and re-tuned.
// drop (-drop d): the context's decode setting (picsong_ctx_set_decode_drop).
Ctx create_decode_ctx(picsong_params p, int device, int drop = 0)
{
    Ctx ctx;
    const float qs = p.qs;
    if (p.lossy && qs > 1.0f) p.qs = 1.0f;
    CK(picsong_ctx_create(&p, device, &ctx.p));
    if (p.lossy && qs > 1.0f) CK(picsong_ctx_set_qs(ctx, qs));
    if (drop > 0) CK(picsong_ctx_set_decode_drop(ctx, drop));
    return ctx;
}

// ---- decoding engine: DecodingEngine::runImage / runVideo call sequence -----------------------
void write_pgm(const std::string &path, const uint8_t *pix, int w, int h, int bit_depth)
{
    // IOManager::writeImage IO/IOManager.ipp:267-344: "P5\n<w> <h>\n<maxval>\n" + w*h bytes
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    f << "P5\n" << w << " " << h << "\n" << ((2 << (bit_depth - 1)) - 1) << "\n";
    f.write(reinterpret_cast<const char *>(pix), (std::streamsize)((size_t)w * h));
}

// ---- RGB decoding (DecodingEngine::runImage / runVideo RGB branches, Engines/DecodingEngine.cu:
// 736-769,868-940): three component streams per frame -> Decode + DWTDecode each -> inverse colour
// transform (offset + clamp fused) -> planar R, G, B planes of W*H bytes appended to <o>
// (IOManager::writeDecodedFrameUChar / writeDecodedFrameComponentUChar, IO/IOManager.ipp:236-262).
// What a decode writes (-reduce r, picsong_reduced_dims): w x h visible pixels a frame of rows pw bytes apart, out of a
// padded image of pw x ph; r = 0: the frame itself (W x H of AW x AH).  win (-window x,y,w,h): the w x h window at
// (x, y) of the image at 1/2^r, rows pw = w bytes apart (ph = h).
struct OutDims { int r, w, h, pw, ph, win = 0, x = 0, y = 0; };

// The frames of an RGB video (-cp 2) in groups of B through ONE call each: picsong_decode_rgb_frames (-reduce r:
// picsong_decode_rgb_frames_reduced; -window: picsong_decode_rgb_frames_window) into planes of od.pw x od.ph bytes, cropped
// on the host, or, -layout (full size only), picsong_decode_rgb_images into the frames as the file takes them -- one pinned
// staging area, one upload and one read-back a group.  The output as frame by frame.
const char *const kShortStream = "Input file is shorter than its _SIZE sidecar says.";
void decode_rgb_groups(const Options &o, const picsong_params &p, picsong_ctx *ctx, hipStream_t s, std::ifstream &in,
                       const std::vector<long> &shorts, long nframes, int aw, int ah, const OutDims &od)
{
    const size_t P = (size_t)od.pw * od.ph, max_shorts = picsong_max_stream_shorts(aw, ah);      // (P: a plane as this call writes it)
    Options og = o;
    og.x = p.width; og.y = p.height;
    const int B = rgb_group_frames(og, P, nframes);
    const size_t raw_bytes = o.layout >= 0 ? layout_frame_bytes(o.layout, p.width, p.height) : 0;
    const size_t frame_bytes = o.layout >= 0 ? raw_bytes : 3 * P;        // a frame of the pixel side
    const auto h_in = pinned_alloc<uint16_t>(max_shorts * 2 * 3 * (size_t)B);
    const auto d_in = dev_alloc<uint16_t>(max_shorts * 2 * 3 * (size_t)B);
    const auto h_pix = pinned_alloc<uint8_t>(frame_bytes * (size_t)B);
    const auto d_pix = dev_alloc<uint8_t>(frame_bytes * (size_t)B);
    std::vector<uint8_t> crop((size_t)od.w * od.h);
    std::ofstream out(o.output, std::ios::binary | std::ios::app);
    size_t pos = 0;
    for (long f = 0; f < nframes; f += B) {
        const int n = (int)std::min<long>(B, nframes - f);
        // the group's 3 n streams are consecutive in the file: one read, a copy each to its place on the device
        size_t group = 0;
        for (int j = 0; j < 3 * n; j++) {
            const size_t len = (size_t)shorts[(size_t)(f * 3 + j)];
            if (len > max_shorts) die("Component codestream longer than the maximum for this geometry.");
            group += len;
        }
        if (!read_exact(in, h_in, group * 2, pos * 2)) die(kShortStream);
        pos += group;
        size_t at = 0;
        for (int j = 0; j < 3 * n; j++) {
            const size_t len = (size_t)shorts[(size_t)(f * 3 + j)];
            HIPCK(hipMemcpyAsync(d_in + (size_t)j * max_shorts, h_in + at, len * 2, hipMemcpyHostToDevice, s));
            at += len;
        }
        if (o.layout >= 0) {
            const picsong_image im = layout_image(o.layout, d_pix, p.width, p.height);
            CK(picsong_decode_rgb_images(ctx, n, d_in, max_shorts, &im, raw_bytes, s));
        } else if (od.win) {
            CK(picsong_decode_rgb_frames_window(ctx, n, d_in, max_shorts, od.r, od.x, od.y, od.w, od.h, d_pix, d_pix + P, d_pix + 2 * P,
                                                (size_t)od.pw, 3 * P, s));
        } else if (od.r > 0) {
            CK(picsong_decode_rgb_frames_reduced(ctx, n, d_in, max_shorts, od.r, d_pix, d_pix + P, d_pix + 2 * P, 3 * P, s));
        } else {
            CK(picsong_decode_rgb_frames(ctx, n, d_in, max_shorts, d_pix, d_pix + P, d_pix + 2 * P, 3 * P, s));
        }
        HIPCK(hipMemcpyAsync(h_pix, d_pix, frame_bytes * (size_t)n, hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
        if (o.layout >= 0) {
            out.write(reinterpret_cast<const char *>(h_pix.p), (std::streamsize)(raw_bytes * (size_t)n));
            continue;
        }
        for (int j = 0; j < 3 * n; j++) {
            crop_rows(crop.data(), h_pix + (size_t)j * P, od.w, od.h, (size_t)od.pw);
            out.write(reinterpret_cast<const char *>(crop.data()), (std::streamsize)crop.size());
        }
    }
}

int run_decode_rgb(const Options &o, const picsong_params &p, picsong_ctx *ctx, std::ifstream &in,
                   const std::vector<long> &shorts, long nframes, int aw, int ah, const OutDims &od)
{
    const size_t P = (size_t)aw * ah, max_shorts = picsong_max_stream_shorts(aw, ah);
    const size_t extra = picsong_dwt_extra(aw, ah, p.wl);
    const Stream s = stream_create();
    const bool batched = p.cp != 3;      // (picsong_decode_rgb_frame: one launch per stage for the three components)
    const auto h_in = pinned_alloc<uint16_t>(max_shorts * 2);
    const auto d_in = dev_alloc<uint16_t>(max_shorts * 2 * (batched ? 3 : 1));
    // -layout: the three padded planes are cropped and interleaved on the device, the frame comes back as the file takes it
    const size_t raw_bytes = o.layout >= 0 ? layout_frame_bytes(o.layout, p.width, p.height) : 0;
    const auto h_pix = pinned_alloc<uint8_t>(raw_bytes > P ? raw_bytes : P);
    const auto d_pix0 = dev_alloc<uint8_t>(3 * P);
    uint8_t *const d_pix[3] = { d_pix0, d_pix0 + P, d_pix0 + 2 * P };
    Dev<uint8_t> d_emit;
    if (o.layout >= 0) d_emit = dev_alloc<uint8_t>(raw_bytes);
    Dev<char> d_plane[3];
    for (int c = 0; c < 3; c++) d_plane[c] = dev_alloc<char>((P + extra) * 4);
    std::vector<uint8_t> crop((size_t)od.w * od.h);
    { std::ofstream trunc(o.output, std::ios::binary | std::ios::trunc); }
    auto t0 = std::chrono::steady_clock::now();
    size_t pos = 0;
    // a video (-cp 2), at full size, reduced or windowed: groups of frames through one call each; everything else frame by
    // frame, here
    const bool grouped = o.video && batched;
    if (grouped) decode_rgb_groups(o, p, ctx, s, in, shorts, nframes, aw, ah, od);
    for (long f = grouped ? nframes : 0; f < nframes; f++) {
        for (int c = 0; c < 3; c++) {
            const size_t n = (size_t)shorts[(size_t)(f * 3 + c)];
            if (n > max_shorts) die("Component codestream longer than the maximum for this geometry.");
            if (!read_exact(in, h_in, n * 2, pos * 2)) die(kShortStream);
            pos += n;
            HIPCK(hipMemcpyAsync(d_in + (batched ? (size_t)c * max_shorts : 0), h_in, n * 2, hipMemcpyHostToDevice, s));
            if (!batched) CK(picsong_decode_plane(ctx, d_in, c, d_plane[c], s));
            HIPCK(hipStreamSynchronize(s));          // h_in (and, plane by plane, d_in) are reused for the next component
        }
        if (od.win)
            CK(picsong_decode_rgb_frame_window(ctx, d_in, max_shorts, od.r, od.x, od.y, od.w, od.h, d_pix[0], d_pix[1],
                                               d_pix[2], (size_t)od.pw, s));
        else if (od.r > 0)
            CK(picsong_decode_rgb_frame_reduced(ctx, d_in, max_shorts, od.r, d_pix[0], d_pix[1], d_pix[2], s));
        else if (batched)
            CK(picsong_decode_rgb_frame(ctx, d_in, max_shorts, d_pix[0], d_pix[1], d_pix[2], s));
        else
            CK(picsong_rgb_inverse(ctx, d_plane[0] + extra * 4, d_plane[1] + extra * 4, d_plane[2] + extra * 4, d_pix[0],
                                   d_pix[1], d_pix[2], s));
        std::ofstream out(o.output, std::ios::binary | std::ios::app);
        if (o.layout >= 0) {
            const picsong_image im = layout_image(o.layout, d_emit, p.width, p.height);
            CK(picsong_emit_frames(ctx, 1, d_pix[0], 0, &im, 0, s));
            HIPCK(hipMemcpyAsync(h_pix, d_emit, raw_bytes, hipMemcpyDeviceToHost, s));
            HIPCK(hipStreamSynchronize(s));
            out.write(reinterpret_cast<const char *>(h_pix.p), (std::streamsize)raw_bytes);
        }
        for (int c = 0; c < 3 && o.layout < 0; c++) {
            HIPCK(hipMemcpyAsync(h_pix, d_pix[c], (size_t)od.pw * od.ph, hipMemcpyDeviceToHost, s));
            HIPCK(hipStreamSynchronize(s));
            crop_rows(crop.data(), h_pix, od.w, od.h, (size_t)od.pw);
            out.write(reinterpret_cast<const char *>(crop.data()), (std::streamsize)crop.size());
        }
    }
    double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::cout << "The time spent with the app without considering allocation periods and I/O is: " << sec << std::endl;
    return 0;
}

// ---- video decode pipeline (DecodingEngine::runVideo, Engines/DecodingEngine.cu:866-1141: reader,
// worker and writer threads).  Every offset is known up front (the _SIZE sidecar gives the stream
// chunks, frames are W*H bytes), so: two reader threads pread chunks into pinned buffers, the main
// thread launches H2D + decode + D2H on the slot's stream, two writer threads wait for their slot's
// stream, crop and pwrite the frame at f * W * H (IOManager::writeDecodedFrame IO/IOManager.ipp:214-231
// appends raw W*H bytes per frame).
int run_decode_video(const Options &o, const picsong_params &p, const std::vector<long> &frame_shorts, long nframes,
                     const OutDims &od)
{
    const int aw = picsong_pad_dim(p.width), ah = picsong_pad_dim(p.height);
    const size_t max_shorts = picsong_max_stream_shorts(aw, ah);
    // (P: the bytes of one decoded, padded frame -- of the reduced image with -reduce)
    const size_t P = (size_t)od.pw * od.ph, frame_bytes = (size_t)od.w * od.h;
    const int nslots = (o.streams < 3 ? 3 : o.streams) + 3;
    // groups of B consecutive frames per launch (picsong_decode_frames), as the encoder's video engine codes them:
    // a 4K frame alone is one decoder wave per SIMD
    const int B = p.cp == 3 ? 1 : frames_per_launch(o.frames_per_launch, (size_t)aw * ah, 16, nframes);
    const long ngroups = (nframes + B - 1) / B;
    struct Slot {
        Ctx ctx; Stream stream;
        Pinned<uint16_t> h_in; Dev<uint16_t> d_in; Pinned<uint8_t> h_pix; Dev<uint8_t> d_pix;
        Dev<uint8_t> d_emit;                             // -layout: the frames cropped on the device, frame_bytes apart
        std::vector<uint8_t> crop;
        int state = 0; long expect = 0;
    };
    enum { FREE = 0, FILLED = 1, LAUNCHED = 2 };
    std::vector<Slot> sl((size_t)nslots);
    for (int i = 0; i < nslots; i++) {
        Slot &k = sl[(size_t)i];
        k.ctx = create_decode_ctx(p, o.device, o.drop);
        load_lut(k.ctx, o, p.wl, 1, p.k, p.cp);
        k.stream = stream_create();
        k.h_in = pinned_alloc<uint16_t>(max_shorts * 2 * B);
        k.d_in = dev_alloc<uint16_t>(max_shorts * 2 * B);
        k.h_pix = pinned_alloc<uint8_t>(P * B);
        k.d_pix = dev_alloc<uint8_t>(P * B);
        if (o.layout >= 0) k.d_emit = dev_alloc<uint8_t>(frame_bytes * (size_t)B);
        else if (od.pw != od.w) k.crop.resize(frame_bytes);
        k.expect = i;
    }
    std::vector<size_t> in_off((size_t)nframes + 1, 0);
    for (long f = 0; f < nframes; f++) {
        if ((size_t)frame_shorts[(size_t)f] > max_shorts) die("Frame codestream longer than the maximum for this geometry.");
        in_off[(size_t)f + 1] = in_off[(size_t)f] + (size_t)frame_shorts[(size_t)f];
    }
    const int ifd = open(o.input.c_str(), O_RDONLY);
    if (ifd < 0) die("Cannot open input file " + o.input);
    const int ofd = open(o.output.c_str(), O_WRONLY | O_CREAT, 0644);
    if (ofd < 0) die("Cannot open output file " + o.output);
    const off_t out_base = lseek(ofd, 0, SEEK_END);          // appended, like the reference
    std::mutex mu;
    std::condition_variable cv;
    std::string failure;
    auto t0 = std::chrono::steady_clock::now();

    auto reader = [&](int r, int nreaders) {
        for (long g = r; g < ngroups; g += nreaders) {
            Slot &k = sl[(size_t)(g % nslots)];
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !failure.empty() || (k.state == FREE && k.expect == g); });
                if (!failure.empty()) return;
            }
            bool short_file = false;
            for (long f = g * B; f < nframes && f < (g + 1) * B; f++)
                if (!pread_exact(ifd, k.h_in + (size_t)(f - g * B) * max_shorts, (size_t)frame_shorts[(size_t)f] * 2, in_off[(size_t)f] * 2))
                    short_file = true;
            std::lock_guard<std::mutex> lk(mu);
            if (short_file && failure.empty()) failure = kShortStream;
            k.state = FILLED;
            cv.notify_all();
        }
    };
    auto writer = [&](int r, int nwriters) {
        (void)hipSetDevice(o.device);
        for (long g = r; g < ngroups; g += nwriters) {
            Slot &k = sl[(size_t)(g % nslots)];
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !failure.empty() || (k.state == LAUNCHED && k.expect == g); });
                if (!failure.empty()) return;
            }
            std::string err;
            if (hipStreamSynchronize(k.stream) != hipSuccess) err = "HIP error while decoding a frame";
            for (long f = g * B; err.empty() && f < nframes && f < (g + 1) * B; f++) {
                const uint8_t *pix = k.h_pix + (size_t)(f - g * B) * (o.layout >= 0 ? frame_bytes : P), *src = pix;
                if (o.layout < 0 && od.pw != od.w) {
                    crop_rows(k.crop.data(), pix, od.w, od.h, (size_t)od.pw);
                    src = k.crop.data();
                }
                if (!pwrite_exact(ofd, src, frame_bytes, (size_t)out_base + (size_t)f * frame_bytes)) err = "Cannot write the output file " + o.output;
            }
            std::lock_guard<std::mutex> lk(mu);
            if (!err.empty() && failure.empty()) failure = err;
            k.state = FREE;
            k.expect = g + nslots;
            cv.notify_all();
        }
    };
    int nreaders = 2, nwriters = 2;
    if (const char *e = getenv("PICSONG_READERS")) { int v = atoi(e); if (v >= 1 && v <= 16) nreaders = v; }
    if (const char *e = getenv("PICSONG_WRITERS")) { int v = atoi(e); if (v >= 1 && v <= 16) nwriters = v; }
    if (nreaders > nslots - 1) nreaders = nslots - 1;
    if (nwriters > nslots - 1) nwriters = nslots - 1;
    std::vector<std::thread> threads;
    for (int r = 0; r < nreaders; r++) threads.emplace_back(reader, r, nreaders);
    for (int r = 0; r < nwriters; r++) threads.emplace_back(writer, r, nwriters);
    for (long g = 0; g < ngroups; g++) {
        Slot &k = sl[(size_t)(g % nslots)];
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !failure.empty() || (k.state == FILLED && k.expect == g); });
            if (!failure.empty()) break;
        }
        const int n = (int)std::min<long>(B, nframes - g * B);
        std::string err;
        for (int b = 0; err.empty() && b < n; b++)
            if (hipMemcpyAsync(k.d_in + (size_t)b * max_shorts, k.h_in + (size_t)b * max_shorts,
                               (size_t)frame_shorts[(size_t)(g * B + b)] * 2, hipMemcpyHostToDevice, k.stream) != hipSuccess)
                err = "HIP error in the codestream upload";
        if (!err.empty()) { }
        else if ((od.win ? picsong_decode_frames_window(k.ctx, n, k.d_in, max_shorts, od.r, od.x, od.y, od.w, od.h, k.d_pix,
                                                        (size_t)od.pw, P, k.stream)
                  : od.r > 0 ? picsong_decode_frames_reduced(k.ctx, n, k.d_in, max_shorts, od.r, k.d_pix, P, k.stream)
                             : picsong_decode_frames(k.ctx, n, k.d_in, max_shorts, k.d_pix, P, k.stream)) != PICSONG_OK)
            err = picsong_last_error();
        else if (o.layout >= 0) {
            const picsong_image im = layout_image(o.layout, k.d_emit, od.w, od.h);
            if (picsong_emit_frames(k.ctx, n, k.d_pix, P, &im, frame_bytes, k.stream) != PICSONG_OK) err = picsong_last_error();
            else if (hipMemcpyAsync(k.h_pix, k.d_emit, frame_bytes * (size_t)n, hipMemcpyDeviceToHost, k.stream) != hipSuccess)
                err = "HIP error in the frame download";
        }
        else if (hipMemcpyAsync(k.h_pix, k.d_pix, P * (size_t)n, hipMemcpyDeviceToHost, k.stream) != hipSuccess)
            err = "HIP error in the frame download";
        std::lock_guard<std::mutex> lk(mu);
        if (!err.empty() && failure.empty()) failure = err;
        k.state = LAUNCHED;
        cv.notify_all();
    }
    for (auto &t : threads) t.join();
    close(ifd);
    close(ofd);
    if (!failure.empty()) die(failure);
    double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::cout << "The time spent with the app without considering allocation periods and I/O is: " << sec << std::endl;
    Options mo = o;
    mo.x = od.w; mo.y = od.h;
    write_metrics(mo, "decode", nframes, sec, 0, 0, 0, (long)in_off[(size_t)nframes]);
    return 0;
}

// -bps 9..16 (the stream's header says so): one grey still image through picsong_decode_images with GREY16, written as
// the 8-bit path writes -- a P5 with maxval 2^bd - 1, its two-byte samples big-endian as Netpbm defines
// ... or, an RGB stream: the frames in groups of B through picsong_decode_rgb_images, appended to the raw output in -layout
int run_decode_deep_rgb(const Options &o, const picsong_params &p, std::ifstream &in)
{
    const long nframes = o.video ? p.frames : 1;
    if (nframes <= 0) die("The header of this stream gives no frames.");
    if (o.frames_per_launch > 21) die(std::string("Incorrect parameters. -framesPerLaunch takes 1..21 RGB frames. ") + kDeepBuilt);
    std::vector<long> shorts;
    {
        std::ifstream sz(o.input + "_SIZE");
        if (!sz) die("Cannot open " + o.input + "_SIZE");
        std::string tok;
        while (std::getline(sz, tok, ',')) if (!tok.empty()) shorts.push_back(std::stol(tok));
        if ((long)shorts.size() < nframes * 3) die("_SIZE sidecar lists fewer streams than the header.");
    }
    HIPCK(hipSetDevice(o.device));
    const Ctx ctx = create_decode_ctx(p, o.device, o.drop);
    load_lut(ctx, o, p.wl, 3, p.k, p.cp);
    int aw, ah, ncb;
    CK(picsong_ctx_padded_dims(ctx, &aw, &ah, &ncb));
    const size_t max_shorts = picsong_max_stream_shorts(aw, ah);
    const int layout16 = deep_rgb_layout(o.layout);
    const size_t fb = deep_rgb_frame_bytes(layout16, p.width, p.height);
    const int B = frames_per_launch(o.frames_per_launch, 6 * (size_t)aw * ah, 21, nframes);
    const Stream s = stream_create();
    const auto h_in = pinned_alloc<uint16_t>(max_shorts * 2 * 3 * (size_t)B);
    const auto d_in = dev_alloc<uint16_t>(max_shorts * 2 * 3 * (size_t)B);
    const auto h_pix = pinned_alloc<uint8_t>(fb * (size_t)B);
    const auto d_pix = dev_alloc<uint8_t>(fb * (size_t)B);
    std::ofstream out(o.output, std::ios::binary | std::ios::trunc);
    if (!out) die("Cannot open output file " + o.output);
    auto t0 = std::chrono::steady_clock::now();
    size_t pos = 0, all = 0;
    for (long f = 0; f < nframes; f += B) {
        const int n = (int)std::min<long>(B, nframes - f);
        size_t group = 0;
        for (int j = 0; j < 3 * n; j++) {
            const size_t len = (size_t)shorts[(size_t)(f * 3 + j)];
            if (len > max_shorts) die("Component codestream longer than the maximum for this geometry.");
            group += len;
        }
        if (!read_exact(in, h_in, group * 2, pos * 2)) die(kShortStream);
        pos += group;
        size_t at = 0;
        for (int j = 0; j < 3 * n; j++) {
            const size_t len = (size_t)shorts[(size_t)(f * 3 + j)];
            HIPCK(hipMemcpyAsync(d_in + (size_t)j * max_shorts, h_in + at, len * 2, hipMemcpyHostToDevice, s));
            at += len;
        }
        const picsong_image im = deep_rgb_image(layout16, d_pix, p.width, p.height);
        CK(picsong_decode_rgb_images(ctx, n, d_in, max_shorts, &im, fb, s));
        HIPCK(hipMemcpyAsync(h_pix, d_pix, fb * (size_t)n, hipMemcpyDeviceToHost, s));
        HIPCK(hipStreamSynchronize(s));
        out.write(reinterpret_cast<const char *>(h_pix.p), (std::streamsize)(fb * (size_t)n));
        all += group;
    }
    double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::cout << "The time spent with the app without considering allocation periods and I/O is: " << sec << std::endl;
    Options mo = o;
    mo.x = p.width; mo.y = p.height;
    write_metrics(mo, "decode_rgb", nframes, sec, 0, 0, 0, (long)all);
    return 0;
}
int run_decode_deep(const Options &o, const picsong_params &p, std::ifstream &in)
{
    deep_check_mode(o, p.is_rgb != 0, p.bit_depth);
    if (p.cp == 3) die(std::string("-cp 3 is not built for -bps 9..16. ") + kDeepBuilt);
    if (p.is_rgb) return run_decode_deep_rgb(o, p, in);
    in.clear();
    in.seekg(0, std::ios::end);
    const size_t shorts = (size_t)in.tellg() / 2;
    HIPCK(hipSetDevice(o.device));
    const Ctx ctx = create_decode_ctx(p, o.device, o.drop);
    load_lut(ctx, o, p.wl, 1, p.k, p.cp);
    int aw, ah, ncb;
    CK(picsong_ctx_padded_dims(ctx, &aw, &ah, &ncb));
    const size_t max_shorts = picsong_max_stream_shorts(aw, ah), n = (size_t)p.width * (size_t)p.height;
    if (shorts > max_shorts) die("Frame codestream longer than the maximum for this geometry.");
    std::vector<uint16_t> stream(max_shorts, 0xFFFFu), img(n);
    in.seekg(0);
    in.read(reinterpret_cast<char *>(stream.data()), (std::streamsize)(shorts * 2));
    const Stream s = stream_create();
    const auto d_in = dev_alloc<uint16_t>(max_shorts * 2);
    const auto d_pix = dev_alloc<uint16_t>(n * 2);
    auto t0 = std::chrono::steady_clock::now();
    HIPCK(hipMemcpyAsync(d_in, stream.data(), max_shorts * 2, hipMemcpyHostToDevice, s));
    picsong_image im;
    im.data = d_pix; im.pitch = (size_t)p.width * 2; im.plane_stride = 0; im.layout = PICSONG_LAYOUT_GREY16;
    CK(picsong_decode_images(ctx, 1, d_in, max_shorts, &im, 0, s));
    HIPCK(hipMemcpyAsync(img.data(), d_pix, n * 2, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (uint16_t &v : img) v = (uint16_t)((v >> 8) | (v << 8));
    {
        std::ofstream f(o.output, std::ios::binary | std::ios::trunc);
        if (!f) die("Cannot open output file " + o.output);
        f << "P5\n" << p.width << " " << p.height << "\n" << ((1 << p.bit_depth) - 1) << "\n";
        f.write(reinterpret_cast<const char *>(img.data()), (std::streamsize)(n * 2));
    }
    std::cout << "The time spent with the app without considering allocation periods and I/O is: " << sec << std::endl;
    Options mo = o;
    mo.x = p.width; mo.y = p.height;
    write_metrics(mo, "decode", 1, sec, 0, 0, 0, (long)shorts);
    return 0;
}

int run_decode(const Options &o)
{
    if (o.input.empty() || o.output.empty()) die("Incorrect parameters. Please choose valid values.");
    std::ifstream in(o.input, std::ios::binary);
    if (!in) die("Cannot open input file " + o.input);
    uint16_t hdr[PICSONG_HDR_SHORTS];
    in.read(reinterpret_cast<char *>(hdr), sizeof hdr);
    if ((size_t)in.gcount() != sizeof hdr) die("Input file too short for a PICSONG header.");
    picsong_params p;
    CK(picsong_header_unpack(hdr, &p));
    if (!((p.components == 1 && !p.is_rgb) || (p.components == 3 && p.is_rgb)))
        die("This stream uses a component layout not built here.");
    if (p.bit_depth != 8) return run_decode_deep(o, p, in);
    layout_check_context(o.layout, p.is_rgb != 0);
    if (o.reduce < 0 || o.reduce > p.wl - 1)
        die("Incorrect parameters. -reduce must lie in 0.." + std::to_string(p.wl - 1) + " (the stream has " +
            std::to_string(p.wl) + " wavelet levels).");
    if (o.drop > 0 && (p.k > 0.0f || p.cp == 3))
        die("Incorrect parameters. -drop applies to -cp 2 streams coded at -k 0 (this one: -cp " + std::to_string(p.cp) + ", -k " +
            std::to_string(p.k) + ").");
    const long nframes = o.video ? p.frames : 1;
    std::vector<long> frame_shorts;
    if (o.video || p.is_rgb) {
        // IOManager::readBulkSizes IO/IOManager.ipp:196-208
        std::ifstream sz(o.input + "_SIZE");
        if (!sz) die("Cannot open " + o.input + "_SIZE");
        std::string tok;
        while (std::getline(sz, tok, ',')) if (!tok.empty()) frame_shorts.push_back(std::stol(tok));
        if ((long)frame_shorts.size() < nframes * p.components) die("_SIZE sidecar lists fewer streams than the header.");
    } else {
        in.seekg(0, std::ios::end);
        frame_shorts.push_back((long)((size_t)in.tellg() / 2));
    }
    HIPCK(hipSetDevice(o.device));
    Ctx ctx = create_decode_ctx(p, o.device, o.drop);
    Options lo = o;
    load_lut(ctx, lo, p.wl, p.components, p.k, p.cp);
    int aw, ah, ncb;
    CK(picsong_ctx_padded_dims(ctx, &aw, &ah, &ncb));
    OutDims od = { o.reduce, 0, 0, 0, 0 };
    CK(picsong_reduced_dims(ctx, o.reduce, &od.w, &od.h, &od.pw, &od.ph, &ncb));
    if (o.win) {                             // the window inside the visible image at 1/2^r, written w x h
        if (p.cp == 3) die("Incorrect parameters. -window does not apply to -cp 3 streams.");
        if ((long)o.wx + o.ww > od.w || (long)o.wy + o.wh > od.h)
            die("Incorrect parameters. -window " + std::to_string(o.wx) + "," + std::to_string(o.wy) + "," +
                std::to_string(o.ww) + "," + std::to_string(o.wh) + " is not inside the " + std::to_string(od.w) + "x" +
                std::to_string(od.h) + " image.");
        CK(picsong_window_codeblocks(ctx, o.reduce, o.wx, o.wy, o.ww, o.wh, &lo.win_cb));
        od.win = 1; od.x = o.wx; od.y = o.wy;
        od.w = od.pw = o.ww; od.h = od.ph = o.wh;
    }
    if (p.is_rgb) return run_decode_rgb(o, p, ctx, in, frame_shorts, nframes, aw, ah, od);
    if (o.video) {
        ctx = Ctx();                         // (the slots of the video pipeline create their own)
        in.close();
        return run_decode_video(lo, p, frame_shorts, nframes, od);
    }
    const size_t P = (size_t)od.pw * od.ph, max_shorts = picsong_max_stream_shorts(aw, ah);
    const Stream s = stream_create();
    const auto h_in = pinned_alloc<uint16_t>(max_shorts * 2);
    const auto d_in = dev_alloc<uint16_t>(max_shorts * 2);
    const auto h_pix = pinned_alloc<uint8_t>(P);
    const auto d_pix = dev_alloc<uint8_t>(P);
    Dev<uint8_t> d_emit;                                 // -layout grey: the frame cropped on the device
    if (o.layout >= 0) d_emit = dev_alloc<uint8_t>((size_t)od.w * od.h);
    std::vector<uint8_t> crop((size_t)od.w * od.h);
    if (o.video) { std::ofstream trunc(o.output, std::ios::binary | std::ios::app); }
    auto t0 = std::chrono::steady_clock::now();
    size_t pos = 0;
    for (long f = 0; f < nframes; f++) {
        const size_t n = (size_t)frame_shorts[(size_t)f];
        if (n > max_shorts) die("Frame codestream longer than the maximum for this geometry.");
        if (!read_exact(in, h_in, n * 2, pos * 2)) die(kShortStream);
        pos += n;
        HIPCK(hipMemcpyAsync(d_in, h_in, n * 2, hipMemcpyHostToDevice, s));
        if (od.win) CK(picsong_decode_frame_window(ctx, d_in, od.r, od.x, od.y, od.w, od.h, d_pix, (size_t)od.pw, s));
        else if (od.r > 0) CK(picsong_decode_frame_reduced(ctx, d_in, od.r, d_pix, s));
        else CK(picsong_decode_frame(ctx, d_in, d_pix, s));
        if (o.layout >= 0) {
            const picsong_image im = layout_image(o.layout, d_emit, od.w, od.h);
            CK(picsong_emit_frames(ctx, 1, d_pix, 0, &im, 0, s));
            HIPCK(hipMemcpyAsync(crop.data(), d_emit, crop.size(), hipMemcpyDeviceToHost, s));
            HIPCK(hipStreamSynchronize(s));
        } else {
            HIPCK(hipMemcpyAsync(h_pix, d_pix, P, hipMemcpyDeviceToHost, s));
            HIPCK(hipStreamSynchronize(s));
            crop_rows(crop.data(), h_pix, od.w, od.h, (size_t)od.pw);
        }
        if (o.video) {
            // IOManager::writeDecodedFrame IO/IOManager.ipp:214-231: raw W*H bytes appended
            std::ofstream out(o.output, std::ios::binary | std::ios::app);
            out.write(reinterpret_cast<const char *>(crop.data()), (std::streamsize)crop.size());
        } else {
            write_pgm(o.output, crop.data(), od.w, od.h, p.bit_depth);
        }
    }
    double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::cout << "The time spent with the app without considering allocation periods and I/O is: " << sec << std::endl;
    Options mo = lo;
    mo.x = od.w; mo.y = od.h;
    write_metrics(mo, "decode", nframes, sec, 0, 0, 0, (long)pos);
    return 0;
}

// ---- -cd 1 -compare <file>: the PSNR and SSE of the decoded output, as written, against a file of the same geometry
// and planar layout (raw, or a PGM whose header is skipped), plane by plane through picsong_frames_sse
int run_compare(const Options &o)
{
    std::ifstream in(o.input, std::ios::binary);
    uint16_t hdr[PICSONG_HDR_SHORTS];
    in.read(reinterpret_cast<char *>(hdr), sizeof hdr);
    picsong_params p;
    CK(picsong_header_unpack(hdr, &p));
    const long planes = (o.video ? (long)p.frames : 1) * (long)p.components;
    const size_t plane_bytes = (size_t)p.width * (size_t)p.height;
    auto open_planes = [&](const std::string &name, std::ifstream &f, size_t &base) {
        f.open(name, std::ios::binary);
        if (!f) die("Cannot open " + name);
        f.seekg(0, std::ios::end);
        const size_t size = (size_t)f.tellg();
        if (size < plane_bytes * (size_t)planes) die(name + " is shorter than the decoded output's planes.");
        const Pgm pgm = sniff_pgm(name);
        base = pgm.is_pgm ? pgm.offset : 0;
        if (size - base != plane_bytes * (size_t)planes) die(name + " does not have the decoded output's geometry.");
    };
    std::ifstream fa, fb;
    size_t base_a = 0, base_b = 0;
    open_planes(o.output, fa, base_a);
    open_planes(o.compare, fb, base_b);
    HIPCK(hipSetDevice(o.device));
    const Ctx ctx = create_decode_ctx(p, o.device);
    int aw, ah, ncb;
    CK(picsong_ctx_padded_dims(ctx, &aw, &ah, &ncb));
    const size_t P = (size_t)aw * ah;
    const auto h = pinned_alloc<uint8_t>(2 * P);
    const auto d = dev_alloc<uint8_t>(2 * P);
    const auto d_sse = dev_alloc<uint64_t>(sizeof(uint64_t));
    const auto h_sse = pinned_alloc<uint64_t>(sizeof(uint64_t));
    std::vector<uint8_t> raw(plane_bytes);
    uint64_t sse = 0, dssim = 0, windows = 0;
    const bool ssim = picsong_ssim_windows(p.width, p.height, &windows) == PICSONG_OK;   // (8 x 8 samples or more)
    for (long i = 0; i < planes; i++) {
        if (!read_exact(fa, raw.data(), plane_bytes, base_a + (size_t)i * plane_bytes)) die("Cannot read back " + o.output);
        CK(picsong_pad_frame_host(raw.data(), p.width, p.height, h, aw, ah));
        if (!read_exact(fb, raw.data(), plane_bytes, base_b + (size_t)i * plane_bytes)) die("Cannot read " + o.compare);
        CK(picsong_pad_frame_host(raw.data(), p.width, p.height, h + P, aw, ah));
        HIPCK(hipMemcpyAsync(d, h, 2 * P, hipMemcpyHostToDevice, nullptr));
        CK(picsong_frames_sse(ctx, 1, d, 0, d + P, 0, d_sse, nullptr));
        HIPCK(hipMemcpyAsync(h_sse, d_sse, sizeof(uint64_t), hipMemcpyDeviceToHost, nullptr));
        HIPCK(hipStreamSynchronize(nullptr));
        sse += *h_sse;
        if (ssim) {
            CK(picsong_frames_dssim(ctx, 1, d, 0, d + P, 0, d_sse, nullptr));
            HIPCK(hipMemcpyAsync(h_sse, d_sse, sizeof(uint64_t), hipMemcpyDeviceToHost, nullptr));
            HIPCK(hipStreamSynchronize(nullptr));
            dssim += *h_sse;
        }
    }
    double psnr = 0.0;
    CK(picsong_sse_to_psnr(sse, (uint64_t)plane_bytes * (uint64_t)planes, &psnr));
    std::cout << "Compare: PSNR " << psnr << " dB, SSE " << sse << " over " << planes << " plane(s) of " << p.width << "x" << p.height
              << std::endl;
    if (ssim) {
        double v = 0.0;
        CK(picsong_dssim_to_ssim(dssim, windows * (uint64_t)planes, &v));
        std::cout << "Compare: SSIM " << ssim_text(v) << ", DSSIM sum " << dssim << " over " << planes << " plane(s)" << std::endl;
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    auto start = std::chrono::steady_clock::now();
    Args a(argc, argv);
    if (a.has("-h") || argc == 1) { help(); return 0; }
    Options o = parse(a);
    int rc;
    if (o.cd == 0) rc = run_encode(o);
    else if (o.cd == 1) { rc = run_decode(o); if (rc == 0 && !o.compare.empty()) rc = run_compare(o); }
    else die("Incorrect parameters. Please choose valid values.");
    double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
    std::cout << "The time spent with the app is: " << sec << std::endl;
    return rc;
}
