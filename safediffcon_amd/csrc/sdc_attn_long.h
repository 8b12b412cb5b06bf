// Streaming softmax attention past 256 tokens (csrc/sdc_attn_long.hip): the entry points sdc_attn / sdc_attn_bwd /
// sdc_attn_bwd_bytes hand over to once they have checked the domain (no rot, no bias, tokens contiguous in qkv and out,
// 256 < ntok <= SDC_ATTN_LONG_MAX).  Internal to libsdc_hip.so: no C export.
#pragma once
#include <cstddef>
#include <cstdint>

namespace sdc {

// Largest ntok of the streaming kernels.  Nothing in them binds near it: addresses are 64-bit, the 32-bit quantities are the
// token index (< 2^31), the 1-D grid outer*inner*heads*ceil(ntok/128) (checked < 2^31 per call) and the row index of the
// statistics workspace (64-bit).  4096 is the largest size the suite holds against the fp64 reference, so it is the cap.
constexpr int ATTN_LONG_MAX = 4096;

int attn_long(const float* qkv, float* out, int outer, int inner, int heads, int ntok, int64_t q_so, int64_t q_sc, int64_t q_si,
              int64_t o_so, int64_t o_sc, int64_t o_si, void* stream);
size_t attn_long_bwd_bytes(int outer, int inner, int heads, int ntok);
int attn_long_bwd(const float* qkv, const float* dout, float* dqkv, void* work, int outer, int inner, int heads, int ntok,
                  int64_t q_so, int64_t q_sc, int64_t q_si, int64_t o_so, int64_t o_sc, int64_t o_si, void* stream);

}  // namespace sdc
