// TEST INFRASTRUCTURE ONLY -- find_subband_sel (bpc_kernels.hpp), the form of the subband search the k = 0 encoder and the
// statistics kernel call with a lane's first column and its codeblock's first row, over arrays of positions.
#include <hip/hip_runtime.h>

#include "../../cuda-image-and-video-codec_amd/csrc/kernel_select.hpp"

using namespace picsong;

extern "C" void emu_find_subband(const int *x, const int *y, int n, int aw, int ah, int wl, int *level, int *sb)
{
    for (int i = 0; i < n; i++) find_subband_sel(x[i], y[i], aw, ah, wl, level[i], sb[i]);
}
