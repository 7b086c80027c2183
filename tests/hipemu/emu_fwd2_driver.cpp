// TEST INFRASTRUCTURE ONLY -- the forward transform of a call that carries several frames (picsong_encode_frames: frame
// 0's plan with grid.z = frames) on the CPU wave emulator, in the frame paths' int16 form, through the library's own
// launch_fwd_plan (launch_seq.hpp): the plan, the band length (f2_pairs_batched) and the head's kernel are its choice.
#include <hip/hip_runtime.h>

#include "../../cuda-image-and-video-codec_amd/csrc/launch_seq.hpp"

using namespace picsong;

static const emu::Go go{};

extern "C" {

// `frames` u8 frames in_z bytes apart into the coefficient buffers out + z * out_z bytes (int16 Mallat arrays at their
// starts).  Returns bit 0: levels 0 and 1 went through the fused head; bit 1: with the batched calls' band length
// (kF2PairsBatch, an instantiation of its own); bit 2: the 16-bit form applies (0: nothing was run).
int emu_dwt_forward_frames(const uint8_t *in, unsigned long long in_z, void *out, unsigned long long out_z, int aw, int ah,
                           int wl, int lossy, float qs, int frames)
{
    std::vector<FwdLaunch> plan = plan_dwt_forward(in, true, out, aw, ah, wl, qs, true);
    if (!plan_is_c16(plan)) return 0;
    plan_frame_strides(plan, in_z, out_z);
    bool fused01 = false;
    launch_fwd_plan(go, lossy != 0, plan, (unsigned)frames, &fused01);
    const int nb = f2_pairs_batched(plan, lossy != 0, (unsigned)frames);
    return 4 | (fused01 ? 1 : 0) | (fused01 && nb > 0 && nb != kF2Pairs ? 2 : 0);
}

int emu_f2_pairs_batch(void) { return kF2PairsBatch; }
int emu_f2_useful_cols(void) { return kF2Useful; }

}  // extern "C"
