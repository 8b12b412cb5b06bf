// Temporal softmax attention at 64 / 96 / 128 frames on the matrix cores (csrc/sdc_tattn_frames.hip): what the entry points
// sdc_attn / sdc_attn_bwd / sdc_attn_bwd_bytes hand over to once sdc_attn_route has said 4.  Internal to libsdc_hip.so: the
// only C export of that file is sdc_attn_route itself (include/sdc.h).
#pragma once
#include <cstddef>
#include <cstdint>

namespace sdc {

// Workgroup slots of the backward: one bias-gradient partial table (heads x ntok x ntok floats) per slot, so the workspace is
// TATTN_FRAMES_SLOTS * heads * ntok^2 floats (67 MB at 128 frames and 4 heads, where 1024 slots would be 268 MB).  One
// workgroup fits a CU (LDS), the MI355X has 256 CUs.
constexpr int TATTN_FRAMES_SLOTS = 256;

inline bool tattn_frames_ntok(int ntok) { return ntok == 64 || ntok == 96 || ntok == 128; }

int tattn_frames(const float* qkv, float* out, const float* rot, const float* bias, int outer, int inner, int heads, int ntok,
                 int64_t q_so, int64_t q_sc, int64_t q_st, int64_t o_so, int64_t o_sc, int64_t o_st, void* stream);
size_t tattn_frames_bwd_bytes(int heads, int ntok);
// dbias_part: null, or the workspace the partial tables go to ([*nslots][heads][ntok][ntok], summed by the caller)
int tattn_frames_bwd(const float* qkv, const float* dout, const float* rot, const float* bias, float* dqkv, float* dbias_part,
                     int* nslots, int outer, int inner, int heads, int ntok, int64_t q_so, int64_t q_sc, int64_t q_st,
                     int64_t o_so, int64_t o_sc, int64_t o_st, void* stream);

}  // namespace sdc
