// Device-side argument blocks of the DCTAutoencoder transformer kernels
// (dctae_model.hip); the C ABI is in include/dctae.h (dctae_model_*).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dctae.h"

namespace dctae {

enum { LIN_F32 = 0, LIN_BF16 = 1, LIN_BF16_QGELU = 2, LIN_F32_RESIDUAL = 3 };

struct LinearArgs {
  const uint16_t* x;   // (M, ldx) bf16, K-contiguous, K % 64 == 0 valid columns
  const uint16_t* w;   // (Nw, ldw) bf16 (nn.Linear weight layout), K columns
  const float* bias;   // (N) or null
  void* out;           // (M, ldo) f32 or bf16 per epilogue
  int64_t M, ldx, ldw, ldo;
  int32_t N, Nw, K;
};

struct AttnArgs {
  const uint16_t* qkv;     // (R * S, 3 * heads * 64) bf16: q | k | v
  const int64_t* ids;      // (R, S) batched_image_ids
  const uint8_t* key_pad;  // (R, S) key_pad_mask (True = pad)
  uint16_t* out;           // (R * S, ldo) bf16, head h at columns 64 h
  int32_t R, S, heads, ldo;
  float scale;             // d_head ** -0.5
  float* lse;              // (R, heads, S) f32 log-sum-exp in log2 units (training forward), or null
};

struct LnArgs {
  const float* x;
  const float* gamma;
  const float* beta;
  uint16_t* out_bf16;      // LayerNorm -> bf16, or
  float* out_f32;          // LayerNorm + position terms -> f32 (embedding)
  const float* pos_h;      // (max_patch_h, D)
  const float* pos_w;      // (max_patch_w, D)
  const float* pos_c;      // (C, D)
  const int64_t* ch;       // (M)
  const int64_t* pos;      // (M, 2)
  int64_t M, ldx, ldo;
  int32_t D;
  float eps;
};

struct PosArgs {
  float* x;
  const float* pos_h;
  const float* pos_w;
  const float* pos_c;
  const int64_t* ch;
  const int64_t* pos;
  int64_t M, ldx;
  int32_t D;
};

struct LfqArgs {
  const float* x;     // (M, ldx): ncb * cbd features
  int64_t* codes;     // (M, ncb)
  uint16_t* q_bf16;   // (M, ldq) or null
  float* q_f32;       // (M, ldq) or null
  int64_t M, ldx, ldq;
  int32_t ncb, cbd;
  float scale;
};

// backward (dctae_model_bwd.hip)
struct AttnBwdArgs {
  const uint16_t* qkv;     // (R * S, 3 * heads * 64) bf16, the forward's operand
  const uint16_t* out;     // (R * S, ldo) bf16, the forward's result
  const uint16_t* dout;    // (R * S, lddo) bf16
  const float* lse;        // (R, heads, S) from the training forward (log2 units)
  const int64_t* ids;
  const uint8_t* key_pad;
  float* delta;            // (R, heads, S) scratch: rowsum(dO * O)
  uint16_t* dqkv;          // (R * S, 3 * heads * 64) bf16: dq | dk | dv
  int32_t R, S, heads, ldo, lddo;
  float scale;
};

constexpr int LN_RPW = 8;   // rows per wave of k_ln_bwd: part_g / part_b have ceil(M / LN_RPW) rows

struct LnBwdArgs {
  const float* x;
  const float* gamma;
  const float* dy;
  float* dx;
  float* part_g;           // (ceil(M / LN_RPW), D) partial sums of dy * xhat
  float* part_b;           // ... of dy
  int64_t M, ldx, lddy, lddx;
  int32_t D, accumulate;   // accumulate: dx += (the fp32 gradient stream)
  float eps;
};

void launch_attention_bwd(const AttnBwdArgs& a, hipStream_t s);
void launch_transpose_pack(const uint16_t* x, int64_t ldx, int64_t M, int C, int64_t Mp, uint16_t* out, hipStream_t s);
void launch_colsum(const void* x, int64_t ldx, int64_t M, int N, bool bf16, float* ws, float* out, hipStream_t s);
void launch_layernorm_bwd(const LnBwdArgs& a, hipStream_t s);
void launch_qgelu(const uint16_t* pre, int64_t ldp, int64_t M, int N, uint16_t* out, int64_t ldo, hipStream_t s);
void launch_qgelu_bwd(const uint16_t* df, int64_t lddf, const uint16_t* pre, int64_t ldp, int64_t M, int N, uint16_t* dpre,
                      int64_t lddp, hipStream_t s);
void launch_pos_grad(const float* g, int64_t ldg, int64_t M, int D, const int64_t* idx, int64_t istride, int rows,
                     float* out, hipStream_t s);

// fused optimizer step (dctae_optim.hip); the table is dctae_optim_seg of include/dctae.h
constexpr int64_t OPT_NORM_CHUNK = 16384;   // gradient elements per block of k_gradnorm_partial
constexpr int64_t OPT_FLAT_CHUNK = 4096;    // elements per flat work item of k_adamw_pack
constexpr int OPT_TILE = 64;                // packed work item: OPT_TILE x OPT_TILE elements
void launch_gradnorm(const dctae_optim_seg* segs, int count, int64_t n_blocks, float max_norm, double* ws, float* stats,
                     hipStream_t s);
void launch_adamw_pack(const dctae_optim_seg* segs, int count, int64_t n_work, const dctae_optim_group* groups,
                       int n_groups, const float* stats, hipStream_t s);

void launch_linear(const LinearArgs& a, int epi, hipStream_t s);
void launch_attention(const AttnArgs& a, hipStream_t s);
// variable-length form (include/dctae_model_prefix.h): a.R, a.S, a.ids, a.key_pad and a.lse are not read
void launch_attention_varlen(const AttnArgs& a, int n_seq, int max_len, const int64_t* seq_start, const int32_t* seq_len,
                             hipStream_t s);
// the prefix token gather (dctae_model_prefix.hip); the four frame tables are device arrays of n_frames entries
struct PrefixGatherArgs {
  const int64_t* ids;       // (R, S)
  const uint8_t* key_pad;   // (R, S)
  const int64_t* pos;       // (R, S, 2)
  const int64_t* ch;        // (R, S)
  const void* codes;        // (R, S, ncb) int64 or int16
  const int32_t* frame_row;
  const int64_t* frame_id;
  const int32_t* frame_m;
  const int64_t* frame_start;
  int64_t* out_codes;       // (M, ncb)
  int64_t* out_ch;          // (M)
  int64_t* out_pos;         // (M, 2)
  int32_t S, ncb, codes16;
};
void launch_prefix_tokens(const PrefixGatherArgs& a, int n_frames, hipStream_t s);
void launch_layernorm(const LnArgs& a, hipStream_t s);
void launch_pos_add(const PosArgs& a, hipStream_t s);
void launch_to_bf16(const float* x, int64_t ldx, int64_t M, int K, int Kp, uint16_t* out, hipStream_t s);
void launch_lfq_codes(const LfqArgs& a, hipStream_t s);

}  // namespace dctae
