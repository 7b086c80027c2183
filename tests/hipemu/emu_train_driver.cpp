// TEST INFRASTRUCTURE ONLY -- the training statistics (picsong_train_coeffs) on the CPU wave emulator: bpc_stats_kernel
// with the grid, the scratch and the arguments picsong_hip.hip gives it (select_stats / stats_args, kernel_select.hpp)
// and the same kernel source (train_kernels.hpp), run through the emulator's launcher.
// Built by tests/test_train_emulated.py with the flags of tests/hipemu/Makefile.
#include <hip/hip_runtime.h>

#include "../../cuda-image-and-video-codec_amd/csrc/launch_seq.hpp"

using namespace picsong;

static const emu::Go go{};

extern "C" {

// coef: `frames` Mallat arrays coef_z bytes apart (form: 0 = int32, 1 = float, 2 = int16); geo: LutGeo's nine fields,
// section sizes of 0 derived for wl; counts: uint64[entries][2], added to.  max_wgs > 0 caps the persistent grid (a
// wave then takes several pairs).  Returns the entries, or -1 for a geometry the kernel's LDS copy cannot hold.
int emu_train_counts(const void *coef, int form, int aw, int ah, int wl, const int *geo, int frames,
                     unsigned long long coef_z, unsigned long long *counts, int *flag, int max_wgs)
{
    LutGeo g = lut_geo(geo);
    lut_geo_sections(g, wl);
    const int total = g.nRef + g.nSig + g.nSign;
    if (total > kTrainMaxEntries) return -1;
    const size_t pairs = (size_t)frames * (size_t)(((aw / 64) * (ah / 64) + 1) / 2);
    StatsLaunch l = select_stats(pairs);
    if (max_wgs > 0 && l.wgs > (unsigned)max_wgs) {
        l.wgs = (unsigned)max_wgs;
        l.scratch_dwords = (size_t)l.wgs * kTrainWgWaves * kEncScratchDwordsPerWave;
    }
    std::vector<uint32_t> ps(l.scratch_dwords, 0xDEADBEEFu);
    const BpcArgs a = stats_args(aw, ah, wl, g, flag, coef, form == 1, form == 2, frames, coef_z, ps.data());
    go(l.kernel, dim3(l.wgs), l.threads, a, counts, (int)pairs);
    return total;
}

int emu_train_max_entries(void) { return kTrainMaxEntries; }

}  // extern "C"
