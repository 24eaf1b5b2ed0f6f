// attention_mh.h -- the two forms behind include/stk_attention_mh.h: the short one lives beside its kernels in
// attention.hip, the streaming one and the entries themselves in attention_long.hip.  Arguments as in the public header;
// the callers have checked the pointers for NULL.
#pragma once

namespace stk_mh {

bool short_ok(int B, int C, int T, int heads);
int short_fwd(const float* q, const float* k, const float* v, long qkv_bstride, float* o, float* lse, float* rec, int B, int C,
              int T, int heads, float scale, void* stream);
int short_bwd(const float* q, const float* k, const float* v, long qkv_bstride, const float* d_o, const float* lse, float* rec,
              float* delta, float* dq, float beta_q, float* dk, float beta_k, float* dv, float beta_v, long grad_bstride, int B,
              int C, int T, int heads, float scale, void* stream);

}  // namespace stk_mh
