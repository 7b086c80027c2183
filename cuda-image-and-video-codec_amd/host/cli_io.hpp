// The file rules of the PICSONG command-line tool that need no GPU: exact reads and writes at an offset, the crop of a
// padded plane, the <o>_SIZE sidecar, the frames-per-launch rule and the P5 sniffer.  No HIP in here: the header compiles
// stand-alone (tests/test_cli_io_host.py).
#pragma once

#include <unistd.h>

#include <cctype>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <string>

namespace cli_io {

// exactly n bytes at `off` of an fd, or false (a short file, an error)
inline bool pread_exact(int fd, void *dst, size_t n, size_t off)
{
    for (size_t got = 0; got < n;) {
        const ssize_t m = pread(fd, static_cast<char *>(dst) + got, n - got, (off_t)(off + got));
        if (m <= 0) return false;
        got += (size_t)m;
    }
    return true;
}
inline bool pwrite_exact(int fd, const void *src, size_t n, size_t off)
{
    for (size_t done = 0; done < n;) {
        const ssize_t m = pwrite(fd, static_cast<const char *>(src) + done, n - done, (off_t)(off + done));
        if (m <= 0) return false;
        done += (size_t)m;
    }
    return true;
}
// the same of a stream, whatever state an earlier short read left it in
inline bool read_exact(std::ifstream &f, void *dst, size_t n, size_t off)
{
    f.clear();
    f.seekg((std::streamoff)off);
    f.read(static_cast<char *>(dst), (std::streamsize)n);
    return (size_t)f.gcount() == n;
}

// the w x h visible samples of a plane whose rows lie `pitch` bytes apart, rows back to back
inline void crop_rows(uint8_t *dst, const uint8_t *src, int w, int h, size_t pitch)
{
    for (int y = 0; y < h; y++) memcpy(dst + (size_t)y * (size_t)w, src + (size_t)y * pitch, (size_t)w);
}

// <o>_SIZE (IOManager.ipp:176-190): stream lengths in shorts, appended; a comma before every entry but the first this
// run writes
struct SizeList {
    std::ofstream f;
    bool any = false;
    explicit SizeList(const std::string &path) : f(path, std::ios::binary | std::ios::app) {}
    void append(const int *shorts, size_t n)
    {
        for (size_t i = 0; i < n; i++) {
            if (any) f << ",";
            f << shorts[i];
            any = true;
        }
    }
};

// frames a launch takes: `asked` (-framesPerLaunch) or 4 while the planes of a frame fit a padded 4K frame (one coder
// wave per SIMD: four of them fill the GPU like an 8K frame) and 1 above; at most `cap` (what the call takes) and the
// frames there are, at least 1
inline int frames_per_launch(int asked, size_t frame_plane_bytes, int cap, long nframes)
{
    long B = asked > 0 ? asked : (frame_plane_bytes <= (size_t)3840 * 2176 ? 4 : 1);
    if (B > cap) B = cap;
    if (B > nframes) B = nframes;
    return (int)(B < 1 ? 1 : B);
}

struct Pgm { bool is_pgm = false; int w = 0, h = 0, maxval = 0; size_t offset = 0; };

inline Pgm sniff_pgm(const std::string &path)
{
    Pgm p;
    std::ifstream f(path, std::ios::binary);
    char magic[2] = { 0, 0 };
    f.read(magic, 2);
    if (!f || magic[0] != 'P' || magic[1] != '5') return p;
    int vals[3], n = 0;
    while (n < 3 && f) {
        int c = f.peek();
        if (c == '#') { std::string line; std::getline(f, line); continue; }
        if (isspace(c)) { f.get(); continue; }
        f >> vals[n++];
    }
    if (n < 3) return p;
    f.get();                                   // single whitespace after maxval
    p.is_pgm = true; p.w = vals[0]; p.h = vals[1]; p.maxval = vals[2]; p.offset = (size_t)f.tellg();
    return p;
}

}  // namespace cli_io
