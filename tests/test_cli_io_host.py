"""cuda-image-and-video-codec_amd/host/cli_io.hpp: the file rules of the command-line tool that need no GPU, exercised by
a stand-alone program (its own main, no HIP) built with -fsanitize=address,undefined and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda-image-and-video-codec_amd", "host")

PROGRAM = r"""
#include "cli_io.hpp"

#include <fcntl.h>
#include <signal.h>
#include <sys/resource.h>

#include <cstdio>
#include <sstream>
#include <vector>

using namespace cli_io;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static std::string slurp(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    std::stringstream s;
    s << f.rdbuf();
    return s.str();
}
static void spit(const std::string &path, const std::string &bytes)
{
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    f.write(bytes.data(), (std::streamsize)bytes.size());
}

int main(int argc, char **argv)
{
    const std::string dir = argv[1];
    std::string hundred;
    for (int i = 0; i < 100; i++) hundred.push_back((char)(i + 1));
    spit(dir + "/hundred", hundred);

    // exact reads: inside the file, up to its last byte, and across its end (an fd, then a stream)
    {
        const int fd = open((dir + "/hundred").c_str(), O_RDONLY);
        EXPECT(fd >= 0);
        std::vector<char> got(40), big(60);
        EXPECT(pread_exact(fd, got.data(), 40, 50) && std::string(got.data(), 40) == hundred.substr(50, 40));
        EXPECT(pread_exact(fd, got.data(), 40, 60) && got[39] == (char)100);
        EXPECT(!pread_exact(fd, big.data(), 60, 50));
        EXPECT(!pread_exact(fd, got.data(), 1, 100));
        EXPECT(pread_exact(fd, got.data(), 0, 100));
        close(fd);
        std::ifstream f(dir + "/hundred", std::ios::binary);
        EXPECT(read_exact(f, got.data(), 40, 50) && std::string(got.data(), 40) == hundred.substr(50, 40));
        EXPECT(!read_exact(f, big.data(), 60, 50));
        EXPECT(read_exact(f, got.data(), 40, 60) && got[39] == (char)100);        // (the short read before it left eof set)
    }
    // the _SIZE writer over 0, 1 and 3 entries, appended twice: a comma before every entry but the first
    {
        const int v[6] = { 7, 12345, 0, 9, 10, 2147483647 };
        const char *want[4] = { "", "7,12345", "", "7,12345,0,9,10,2147483647" };
        for (int c : { 0, 1, 3 }) {
            const std::string path = dir + "/size" + std::to_string(c);
            {
                SizeList s(path);
                s.append(v, (size_t)c);
                s.append(v + c, (size_t)c);
            }
            EXPECT(slurp(path) == want[c]);
        }
        // ... of what one run writes: a second run appends to the file as it is (IOManager.ipp:176-190 does)
        { SizeList s(dir + "/size1"); s.append(v + 2, 1); }
        EXPECT(slurp(dir + "/size1") == "7,123450");
    }
    // a crop from pitch 192 to width 136
    {
        const int w = 136, h = 5, pitch = 192;
        std::vector<uint8_t> src((size_t)pitch * h), dst((size_t)w * h, 0);
        for (size_t i = 0; i < src.size(); i++) src[i] = (uint8_t)(i % pitch < (size_t)w ? (i * 7 + 3) & 0xFF : 0xEE);
        crop_rows(dst.data(), src.data(), w, h, pitch);
        bool same = true;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) same = same && dst[(size_t)y * w + x] == src[(size_t)y * pitch + x];
        EXPECT(same);
    }
    // frames per launch: 4 up to a padded 4K frame's 3840 x 2176 bytes and 1 above, -framesPerLaunch instead, both caps,
    // the frames there are, never less than 1
    {
        const size_t k4 = (size_t)3840 * 2176;
        EXPECT(frames_per_launch(0, k4, 16, 100) == 4);
        EXPECT(frames_per_launch(0, k4 + 1, 16, 100) == 1);
        EXPECT(frames_per_launch(0, 3 * (k4 / 3), 21, 100) == 4);              // (an RGB frame: its three planes)
        EXPECT(frames_per_launch(0, 3 * (k4 / 3 + 1), 21, 100) == 1);
        EXPECT(frames_per_launch(2, k4 + 1, 16, 100) == 2);
        EXPECT(frames_per_launch(16, k4, 16, 100) == 16);
        EXPECT(frames_per_launch(17, k4, 16, 100) == 16);
        EXPECT(frames_per_launch(21, k4, 21, 100) == 21);
        EXPECT(frames_per_launch(40, k4, 21, 100) == 21);
        EXPECT(frames_per_launch(0, 1, 16, 3) == 3);
        EXPECT(frames_per_launch(8, 1, 16, 5) == 5);
        EXPECT(frames_per_launch(0, 1, 16, 0) == 1);
    }
    // P5 sniffing: a comment line, maxval 255 and 65535; what is no PGM
    {
        const std::string h8 = "P5\n# made by a test\n200 136\n255\n", h16 = "P5 200\n136 # depth\n65535\n";
        spit(dir + "/a.pgm", h8 + hundred);
        spit(dir + "/b.pgm", h16 + hundred);
        const Pgm a = sniff_pgm(dir + "/a.pgm"), b = sniff_pgm(dir + "/b.pgm");
        EXPECT(a.is_pgm && a.w == 200 && a.h == 136 && a.maxval == 255 && a.offset == h8.size());
        EXPECT(b.is_pgm && b.w == 200 && b.h == 136 && b.maxval == 65535 && b.offset == h16.size());
        EXPECT(!sniff_pgm(dir + "/hundred").is_pgm);
        EXPECT(!sniff_pgm(dir + "/missing").is_pgm);
        spit(dir + "/c.pgm", "P5\n200");
        EXPECT(!sniff_pgm(dir + "/c.pgm").is_pgm);
    }
    // exact writes: inside and behind the file; across the largest size the file may take (RLIMIT_FSIZE), which fails
    {
        const int fd = open((dir + "/hundred").c_str(), O_WRONLY);
        EXPECT(fd >= 0);
        EXPECT(pwrite_exact(fd, "abcd", 4, 10) && pwrite_exact(fd, "wxyz", 4, 98));
        const std::string now = slurp(dir + "/hundred");
        EXPECT(now.size() == 102 && now.substr(10, 4) == "abcd" && now.substr(96, 6) == std::string("\x61\x62", 2) + "wxyz");
        signal(SIGXFSZ, SIG_IGN);
        const rlimit lim = { 120, 120 };
        EXPECT(setrlimit(RLIMIT_FSIZE, &lim) == 0);
        EXPECT(pwrite_exact(fd, hundred.data(), 18, 102));
        EXPECT(!pwrite_exact(fd, hundred.data(), 40, 100));
        EXPECT(!pwrite_exact(fd, hundred.data(), 1, 120));
        close(fd);
        EXPECT(!pwrite_exact(-1, "a", 1, 0));
    }
    if (!failures) std::printf("CLI_IO OK\n");
    return failures ? 1 : 0;
}
"""


def test_cli_io_header_stands_alone_under_sanitizers(tmp_path):
    src, exe, work = tmp_path / "cli_io_check.cpp", tmp_path / "cli_io_check", tmp_path / "work"
    src.write_text(PROGRAM)
    work.mkdir()
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", HOST, "-o", str(exe), str(src)])
    r = subprocess.run([str(exe), str(work)], capture_output=True, text=True)
    assert r.returncode == 0 and "CLI_IO OK" in r.stdout and not r.stderr, r.stdout + r.stderr
