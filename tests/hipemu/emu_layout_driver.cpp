// TEST INFRASTRUCTURE ONLY -- the pixel-layout kernels (layout_kernels.hpp) on the CPU wave emulator: the argument check
// (layout_refusal, kernel_select.hpp), and ingest_kernel / emit_kernel through the launch sequences the library runs
// (ingest_frames / emit_frames, launch_seq.hpp).
// Built by tests/test_layout_emulated.py with the flags of tests/hipemu/Makefile.
#include <hip/hip_runtime.h>

#include <sys/mman.h>
#include <unistd.h>

#include "../../cuda-image-and-video-codec_amd/csrc/launch_seq.hpp"

using namespace picsong;

static const emu::Go go{};

extern "C" {

// 1 and the reason in msg when the calls refuse these arguments, else 0
int emu_layout_refusal(int layout, const void *data, unsigned long long pitch, unsigned long long plane_stride,
                       unsigned long long frame_stride, const void *padded, unsigned long long padded_stride, int n, int w, int h, int aw,
                       int ah, char *msg, int cap)
{
    const char *why = layout_refusal(layout, data, (size_t)pitch, (size_t)plane_stride, (size_t)frame_stride, padded, (size_t)padded_stride,
                                     n, w, h, aw, ah);
    if (msg && cap > 0) snprintf(msg, (size_t)cap, "%s", why ? why : "");
    return why ? 1 : 0;
}

// -1: refused (nothing run); else 1 when the vector form ran, 0 for the per-byte one
int emu_ingest(int layout, const void *data, unsigned long long pitch, unsigned long long plane_stride, unsigned long long frame_stride,
               uint8_t *padded, unsigned long long padded_stride, int n, int w, int h, int aw, int ah)
{
    if (layout_refusal(layout, data, (size_t)pitch, (size_t)plane_stride, (size_t)frame_stride, padded, (size_t)padded_stride, n, w, h, aw, ah))
        return -1;
    bool vec = false;
    if (ingest_frames(go, layout, data, (size_t)pitch, (size_t)plane_stride, (size_t)frame_stride, padded, (size_t)padded_stride, n, w, h,
                      aw, ah, &vec)) return -1;
    return vec ? 1 : 0;
}

int emu_emit(int layout, const uint8_t *padded, unsigned long long padded_stride, void *data, unsigned long long pitch,
             unsigned long long plane_stride, unsigned long long frame_stride, int n, int w, int h, int aw, int ah)
{
    if (layout_refusal(layout, data, (size_t)pitch, (size_t)plane_stride, (size_t)frame_stride, padded, (size_t)padded_stride, n, w, h, aw, ah))
        return -1;
    bool vec = false;
    if (emit_frames(go, layout, padded, (size_t)padded_stride, data, (size_t)pitch, (size_t)plane_stride, (size_t)frame_stride, n, w, h, aw,
                    ah, &vec)) return -1;
    return vec ? 1 : 0;
}

// n bytes whose last one is the last byte of a page, the page behind it without access: a read or write past the
// buffer's end is a fault, not a silent one.  (The base's alignment follows from n.)
void *emu_guard_alloc(unsigned long long n)
{
    const size_t page = (size_t)sysconf(_SC_PAGESIZE), body = ((size_t)n + page - 1) / page * page;
    char *m = (char *)mmap(nullptr, body + page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == MAP_FAILED) return nullptr;
    if (mprotect(m + body, page, PROT_NONE) != 0) { munmap(m, body + page); return nullptr; }
    return m + body - (size_t)n;
}
void emu_guard_free(void *p, unsigned long long n)
{
    const size_t page = (size_t)sysconf(_SC_PAGESIZE), body = ((size_t)n + page - 1) / page * page;
    munmap((char *)p + (size_t)n - body, body + page);
}

}  // extern "C"
