// moolib_amd._kernels — hand-written HIP/CDNA4 (gfx950) kernels for the
// IMPALA hot path.
//
// Kernel inventory (BASELINE.json north star: "the V-trace
// returns/advantages scan, the policy-gradient + entropy loss ... are
// hand-written CDNA4 HIP kernels"):
//   vtrace_scan_kernel     — fused V-trace backward scan + pg-advantages.
//     The reference computes this with a T-step Python loop of torch ops
//     (examples/common/vtrace.py:221-227): ~6 kernel launches per timestep
//     (~120 for T=20). Here it is ONE launch; each lane owns a batch
//     column, the T-recursion runs in registers. [T,B] is tiny (20x32), so
//     this is launch-latency elimination, not FLOPs.
//   impala_loss_fwd_kernel — fused pg + entropy + baseline loss forward AND
//     d(logits)/d(baseline) in a single pass over [N=T*B, A] rows: one
//     wavefront per row computes softmax/log-softmax via wave reductions
//     and writes the combined logits gradient directly (saves the autograd
//     graph + ~15 separate elementwise/softmax kernels of the eager path).
//   r2d2_loss_kernel (r2d2.hip.inc) — fused R2D2 loss: n-step double-Q
//     targets under value rescaling, masked sequence loss, sequence
//     priorities and d(loss)/d(q) in one launch, no atomics.
//   actor_priority_kernel (r2d2.hip.inc) — the actor's initial sequence
//     priorities from its own q_taken / q_max, one launch.
//   act_categorical_kernel, act_eps_greedy_kernel (act.hip.inc) — the actor's
//     action head: Philox4x32-10 sampling from a [seed, step] state on the
//     device, one launch each.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include <climits>
#include <cstdlib>
#include <vector>

#define DEV_INLINE __device__ __forceinline__

namespace {

constexpr int kWave = 64;

// ------------------------------------------------------------- V-trace

__global__ void vtrace_scan_kernel(const float* __restrict__ log_rhos,
                                   const float* __restrict__ discounts,
                                   const float* __restrict__ rewards,
                                   const float* __restrict__ values,
                                   const float* __restrict__ bootstrap,
                                   float* __restrict__ vs,
                                   float* __restrict__ pg_advantages, int T, int B,
                                   float rho_bar, float pg_rho_bar) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;

  // Backward scan: A_t = delta_t + gamma_t c_t A_{t+1}; vs_t = A_t + V_t.
  float acc = 0.f;
  for (int t = T - 1; t >= 0; --t) {
    int i = t * B + b;
    float rho = __expf(log_rhos[i]);
    float crho = rho_bar > 0.f ? fminf(rho, rho_bar) : rho;
    float c = fminf(rho, 1.f);
    float next_v = (t == T - 1) ? bootstrap[b] : values[i + B];
    float disc = discounts[i];
    float delta = crho * (rewards[i] + disc * next_v - values[i]);
    acc = delta + disc * c * acc;
    vs[i] = acc + values[i];
  }
  // Forward pass for pg advantages: uses vs_{t+1}.
  for (int t = 0; t < T; ++t) {
    int i = t * B + b;
    float rho = __expf(log_rhos[i]);
    float pgrho = pg_rho_bar > 0.f ? fminf(rho, pg_rho_bar) : rho;
    float next_vs = (t == T - 1) ? bootstrap[b] : vs[i + B];
    pg_advantages[i] = pgrho * (rewards[i] + discounts[i] * next_vs - values[i]);
  }
}

// -------------------------------------------------- fused IMPALA losses

DEV_INLINE float waveReduceSum(float v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
  return __shfl(v, 0);
}
DEV_INLINE float waveReduceMax(float v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off));
  return __shfl(v, 0);
}

// One wavefront per row (row = one (t,b) position, A actions).
// Computes, per row:
//   entropy contribution  H = -sum p log p            (loss -H * entropy_cost)
//   pg contribution       -logp[a] * adv
//   and d total_loss / d logits  written to grad_logits:
//     d(-mean H)/dlogit_j * ec = ec/N * p_j*(logp_j + H)
//     d(pg)/dlogit_j           = adv/N * (p_j - 1[j==a])
// Baseline loss/grad are elementwise and handled on the [T,B] tensors:
//   loss_b = bc * 0.5/N * (vs - baseline)^2 ; dbaseline = bc/N*(baseline-vs)
__global__ void impala_loss_kernel(const float* __restrict__ logits,
                                   const int64_t* __restrict__ actions,
                                   const float* __restrict__ pg_advantages,
                                   const float* __restrict__ vs,
                                   const float* __restrict__ baseline,
                                   float* __restrict__ grad_logits,
                                   float* __restrict__ grad_baseline,
                                   float* __restrict__ loss_parts,  // [3]: pg, baseline, entropy
                                   int N, int A, float entropy_cost, float baseline_cost,
                                   float grad_scale) {
  int row = blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
  int lane = threadIdx.x % kWave;
  if (row >= N) return;
  const float* lrow = logits + (int64_t)row * A;
  float* grow = grad_logits + (int64_t)row * A;

  float m = -INFINITY;
  for (int j = lane; j < A; j += kWave) m = fmaxf(m, lrow[j]);
  m = waveReduceMax(m);
  float z = 0.f;
  for (int j = lane; j < A; j += kWave) z += __expf(lrow[j] - m);
  z = waveReduceSum(z);
  float logz = __logf(z) + m;

  // entropy H = -sum p logp = logz - sum p*logit... compute directly
  float h = 0.f;
  for (int j = lane; j < A; j += kWave) {
    float lp = lrow[j] - logz;
    h -= __expf(lp) * lp;
  }
  h = waveReduceSum(h);

  int64_t a = actions[row];
  // Defensive clamp: an out-of-range action (corrupted input) must not
  // fault the GPU; training numerics elsewhere will surface the bug.
  if (a < 0 || a >= A) a = 0;
  float adv = pg_advantages[row];
  float logp_a = lrow[a] - logz;

  float inv_n = 1.f / N;
  for (int j = lane; j < A; j += kWave) {
    float p = __expf(lrow[j] - logz);
    float lp = lrow[j] - logz;
    float g_ent = entropy_cost * inv_n * p * (lp + h);
    float g_pg = adv * inv_n * (p - (j == (int)a ? 1.f : 0.f));
    grow[j] = (g_ent + g_pg) * grad_scale;
  }

  float diff = baseline[row] - vs[row];
  grad_baseline[row] = baseline_cost * inv_n * diff * grad_scale;

  if (lane == 0) {
    atomicAdd(&loss_parts[0], -logp_a * adv * inv_n);
    atomicAdd(&loss_parts[1], baseline_cost * 0.5f * diff * diff * inv_n);
    atomicAdd(&loss_parts[2], -entropy_cost * h * inv_n);
  }
}

// ------------------------------------------------- NHWC max pooling 3x3/2
//
// The IMPALA ResNet's three pools (84->42->21->11, k3 s2 p1). torch's NHWC
// maxpool backward scatters with atomics (~186 us on [672,16,42,42] grads);
// this pair stores a window index in the forward and GATHERS in the
// backward (each input element checks its <=4 covering windows) — no
// atomics, bandwidth-bound.

// Vectorized over 8 NHWC channels per thread: all loads/stores are 16-byte
// (bf16x8) or 8-byte (idx) contiguous chunks.
template <typename T>
struct Vec8 {
  T v[8];
};

template <typename T>
__global__ void maxpool3x3s2_fwd_kernel(const T* __restrict__ in, T* __restrict__ out,
                                        uint8_t* __restrict__ idx, int N, int H, int W, int C,
                                        int OH, int OW) {
  int C8 = C >> 3;
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)N * OH * OW * C8;
  if (tid >= total) return;
  int c8 = tid % C8;
  int64_t t = tid / C8;
  int ow = t % OW;
  t /= OW;
  int oh = t % OH;
  int n = t / OH;

  float best[8];
  int besti[8];
  // Start at the first IN-BOUNDS tap (tap 0 is padding for the first output
  // row/column): a window whose values are all -inf never takes the branch
  // below and must still route its gradient to a real input element, the
  // first one in scan order like torch.
  const int firstTap = (oh == 0 ? 3 : 0) + (ow == 0 ? 1 : 0);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    best[j] = -INFINITY;
    besti[j] = firstTap;
  }
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    int ih = oh * 2 - 1 + kh;
    if (ih < 0 || ih >= H) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      int iw = ow * 2 - 1 + kw;
      if (iw < 0 || iw >= W) continue;
      const Vec8<T> vin =
          *reinterpret_cast<const Vec8<T>*>(in + ((((int64_t)n * H + ih) * W + iw) * C8 + c8) * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = (float)vin.v[j];
        if (v > best[j] || v != v) {  // NaN propagates, as in torch
          best[j] = v;
          besti[j] = kh * 3 + kw;
        }
      }
    }
  }
  Vec8<T> vout;
  Vec8<uint8_t> vidx;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    vout.v[j] = (T)best[j];
    vidx.v[j] = (uint8_t)besti[j];
  }
  *reinterpret_cast<Vec8<T>*>(out + tid * 8) = vout;
  *reinterpret_cast<Vec8<uint8_t>*>(idx + tid * 8) = vidx;
}

template <typename T>
__global__ void maxpool3x3s2_bwd_kernel(const T* __restrict__ gout,
                                        const uint8_t* __restrict__ idx, T* __restrict__ gin,
                                        int N, int H, int W, int C, int OH, int OW) {
  int C8 = C >> 3;
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)N * H * W * C8;
  if (tid >= total) return;
  int c8 = tid % C8;
  int64_t t = tid / C8;
  int iw = t % W;
  t /= W;
  int ih = t % H;
  int n = t / H;

  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  int oh_lo = (ih == 0) ? 0 : ih / 2;  // ceil((ih-1)/2)
  int oh_hi = (ih + 1) / 2;
  int ow_lo = (iw == 0) ? 0 : iw / 2;
  int ow_hi = (iw + 1) / 2;
  for (int oh = oh_lo; oh <= oh_hi && oh < OH; ++oh) {
    int kh = ih - (oh * 2 - 1);
    if (kh < 0 || kh > 2) continue;
    for (int ow = ow_lo; ow <= ow_hi && ow < OW; ++ow) {
      int kw = iw - (ow * 2 - 1);
      if (kw < 0 || kw > 2) continue;
      int64_t o = (((int64_t)n * OH + oh) * OW + ow) * C8 + c8;
      const Vec8<uint8_t> vidx = *reinterpret_cast<const Vec8<uint8_t>*>(idx + o * 8);
      const Vec8<T> vg = *reinterpret_cast<const Vec8<T>*>(gout + o * 8);
      uint8_t code = (uint8_t)(kh * 3 + kw);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (vidx.v[j] == code) acc[j] += (float)vg.v[j];
      }
    }
  }
  Vec8<T> vout;
#pragma unroll
  for (int j = 0; j < 8; ++j) vout.v[j] = (T)acc[j];
  *reinterpret_cast<Vec8<T>*>(gin + tid * 8) = vout;
}

// -------------------------------------------- frame preprocessing (fused)
//
// uint8 [N,C,H,W] frames -> bf16 NHWC scaled by 1/255, in one pass. The
// eager path (to(dtype) + mul_ + contiguous(channels_last)) is 3 kernels
// over the largest tensor in the network.

__global__ void frames_u8_to_bf16_nhwc_kernel(const uint8_t* __restrict__ in,
                                              hip_bfloat16* __restrict__ out, float scale,
                                              int N, int C, int H, int W, int CO) {
  // CO >= C: output channels beyond C are zero (channel padding so the
  // MFMA conv template, whose A fragments span 8 contiguous channels of
  // one tap, can run the 4-channel first layer as C=8).
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)N * CO * H * W;
  if (tid >= total) return;
  // tid enumerates the OUTPUT (NHWC) layout for coalesced writes.
  int c = tid % CO;
  int64_t t = tid / CO;
  int w = t % W;
  t /= W;
  int h = t % H;
  int n = t / H;
  float v = 0.f;
  if (c < C) v = (float)in[(((int64_t)n * C + c) * H + h) * W + w] * scale;
  out[tid] = (hip_bfloat16)v;
}

// CO == 8 fast path: one thread per PIXEL — C strided byte reads, one
// 16-byte bf16x8 store (the generic kernel's 2-byte scatter stores were
// the cost: 115 us for the 672-image learner batch).
using bf16x8v = __attribute__((ext_vector_type(8))) __bf16;

__global__ __launch_bounds__(256) void frames_u8_pad8_kernel(
    const uint8_t* __restrict__ in, __bf16* __restrict__ out, float scale, int N, int C,
    int64_t HW) {
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)N * HW;
  if (tid >= total) return;
  const int64_t n = tid / HW;
  const int64_t p = tid - n * HW;
  bf16x8v v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (__bf16)0.f;
  const uint8_t* base = in + (n * C) * HW + p;
  for (int c = 0; c < C; ++c) v[c] = (__bf16)((float)base[(int64_t)c * HW] * scale);
  *reinterpret_cast<bf16x8v*>(out + tid * 8) = v;
}

// ------------------------------------------ fused first conv (actor path)
//
// conv1 of the IMPALA ResNet: uint8 NCHW frames -> 3x3 conv (C_in=4,
// C_out=16, pad 1) + bias -> bf16 NHWC, in ONE kernel. At C_in=4 the
// implicit-GEMM K is 36 — far too small for MFMA to pay — and the op is
// VALU/L1-bound, so a direct conv that also folds the uint8 scale (and
// skips the separate preprocessing pass + its 19 MB intermediate) wins.
// One thread per output pixel computes all 16 output channels; the 1.2 KB
// weight block is staged in LDS.

__global__ __launch_bounds__(256) void conv1_u8_nhwc_kernel(const uint8_t* __restrict__ in,   // [N,4,H,W]
                                     const hip_bfloat16* __restrict__ w,  // [3,3,4,16]
                                     const hip_bfloat16* __restrict__ bias,  // [16]
                                     hip_bfloat16* __restrict__ out,  // [N,H,W,16] (NHWC)
                                     float scale, int N, int H, int W) {
  constexpr int CI = 4, CO = 16;
  __shared__ float wsm[3 * 3 * CI * CO];
  __shared__ float bsm[CO];
  for (int i = threadIdx.x; i < 3 * 3 * CI * CO; i += blockDim.x) wsm[i] = (float)w[i];
  for (int i = threadIdx.x; i < CO; i += blockDim.x) bsm[i] = (float)bias[i];
  __syncthreads();

  // 2 output pixels per thread: each (kh, ci) input row contributes a
  // 4-byte span (iw-1..iw+2) fetched as ONE dword in the interior — 12
  // dword loads replace the naive 72 scalar byte loads per 2 pixels.
  const int WT = (W + 1) / 2;  // width tiles
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)N * H * WT;
  if (tid >= total) return;
  int ow0 = (int)(tid % WT) * 2;
  int64_t t = tid / WT;
  int oh = t % H;
  int n = t / H;

  float acc[2][CO];
#pragma unroll
  for (int px = 0; px < 2; ++px)
#pragma unroll
    for (int co = 0; co < CO; ++co) acc[px][co] = bsm[co];

#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    int ih = oh + kh - 1;
    if (ih < 0 || ih >= H) continue;
#pragma unroll
    for (int ci = 0; ci < CI; ++ci) {
      const uint8_t* row = in + (((int64_t)n * CI + ci) * H + ih) * W;
      float xv[4];  // input columns ow0-1 .. ow0+2
      if (ow0 >= 1 && ow0 + 2 < W) {
        uint32_t v;
        __builtin_memcpy(&v, row + ow0 - 1, 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = (float)((v >> (8 * j)) & 0xff) * scale;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          int iw = ow0 - 1 + j;
          xv[j] = (iw >= 0 && iw < W) ? (float)row[iw] * scale : 0.f;
        }
      }
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const float* wp = &wsm[((kh * 3 + kw) * CI + ci) * CO];
#pragma unroll
        for (int px = 0; px < 2; ++px) {
#pragma unroll
          for (int co = 0; co < CO; ++co) {
            acc[px][co] = fmaf(xv[kw + px], wp[co], acc[px][co]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int px = 0; px < 2; ++px) {
    const int ow = ow0 + px;
    if (ow >= W) break;
    hip_bfloat16* op = out + (((int64_t)n * H + oh) * W + ow) * CO;
#pragma unroll
    for (int co = 0; co < CO; ++co) op[co] = (hip_bfloat16)acc[px][co];
  }
}

}  // namespace

#include "conv3x3.hip.inc"
#include "wgrad3x3.hip.inc"
#include "lstm.hip.inc"
#include "r2d2.hip.inc"

// ------------------------------------------------------------ wrappers

// The LSTM kernels index every operand from T and B alone: each one must be
// on X's device, contiguous, and of exactly the dtype and shape the kernel
// reinterprets it as.
static void checkLstmArg(const at::Tensor& t, const at::Tensor& like, at::ScalarType dtype,
                         at::IntArrayRef shape, const char* who, const char* name) {
  TORCH_CHECK(t.defined() && t.is_cuda() && t.device() == like.device(), who, ": ", name,
              " must be on the same CUDA device as the input");
  TORCH_CHECK(t.scalar_type() == dtype, who, ": ", name, " must be ", dtype, ", got ",
              t.scalar_type());
  TORCH_CHECK(t.sizes() == shape, who, ": ", name, " must have shape ", shape, ", got ",
              t.sizes());
  TORCH_CHECK(t.is_contiguous(), who, ": ", name, " must be contiguous");
}

std::vector<at::Tensor> lstm_fused_fwd(at::Tensor X, at::Tensor notdone, at::Tensor h0,
                                       at::Tensor c0, at::Tensor whhPacked) {
  TORCH_CHECK(X.is_cuda() && X.dtype() == at::kBFloat16 && X.dim() == 3, "lstm fwd: X [T,B,4H] bf16");
  TORCH_CHECK(X.is_contiguous(), "lstm fwd: X must be contiguous");
  int T = X.size(0), B = X.size(1);
  TORCH_CHECK(X.size(2) == lstm::kG, "lstm fwd: hidden size must be 256");
  checkLstmArg(notdone, X, at::kFloat, {T, B}, "lstm fwd", "notdone");
  checkLstmArg(h0, X, at::kBFloat16, {B, lstm::kH}, "lstm fwd", "h0");
  checkLstmArg(c0, X, at::kFloat, {B, lstm::kH}, "lstm fwd", "c0");
  checkLstmArg(whhPacked, X, at::kBFloat16, {(int64_t)lstm::kH * lstm::kG}, "lstm fwd",
               "whhPacked");
  auto opts = X.options();
  auto fopts = opts.dtype(at::kFloat);
  auto H = at::empty({T, B, lstm::kH}, opts);
  auto gates = at::empty({T, B, lstm::kG}, opts);
  auto cs = at::empty({T, B, lstm::kH}, fopts);
  auto hT = at::empty({B, lstm::kH}, opts);
  auto cT = at::empty({B, lstm::kH}, fopts);
  int blocks = (B + lstm::kBM - 1) / lstm::kBM;
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(lstm::lstm_fwd_kernel, dim3(blocks), dim3(lstm::kThreads), 0, stream,
                     reinterpret_cast<const lstm::bf16*>(X.data_ptr()),
                     notdone.data_ptr<float>(),
                     reinterpret_cast<const lstm::bf16*>(h0.data_ptr()), c0.data_ptr<float>(),
                     reinterpret_cast<const lstm::bf16*>(whhPacked.data_ptr()),
                     reinterpret_cast<lstm::bf16*>(H.data_ptr()),
                     reinterpret_cast<lstm::bf16*>(gates.data_ptr()), cs.data_ptr<float>(),
                     reinterpret_cast<lstm::bf16*>(hT.data_ptr()), cT.data_ptr<float>(), T, B);
  return {H, gates, cs, hT, cT};
}

std::vector<at::Tensor> lstm_fused_bwd(at::Tensor gates, at::Tensor cs, at::Tensor c0,
                                       at::Tensor notdone, at::Tensor dH, at::Tensor dhT,
                                       at::Tensor dcT, at::Tensor whhPackedN) {
  TORCH_CHECK(gates.is_cuda() && gates.dtype() == at::kBFloat16 && gates.dim() == 3 &&
                  gates.size(2) == lstm::kG && gates.is_contiguous(),
              "lstm bwd: gates [T,B,4H] contiguous bf16");
  int T = gates.size(0), B = gates.size(1);
  checkLstmArg(cs, gates, at::kFloat, {T, B, lstm::kH}, "lstm bwd", "cs");
  checkLstmArg(c0, gates, at::kFloat, {B, lstm::kH}, "lstm bwd", "c0");
  checkLstmArg(notdone, gates, at::kFloat, {T, B}, "lstm bwd", "notdone");
  checkLstmArg(dH, gates, at::kBFloat16, {T, B, lstm::kH}, "lstm bwd", "dH");
  // dhT / dcT: an undefined or EMPTY tensor means "no gradient" (the Python
  // side passes torch.Tensor(), whose data pointer is null)
  if (dhT.defined() && dhT.numel() > 0)
    checkLstmArg(dhT, gates, at::kBFloat16, {B, lstm::kH}, "lstm bwd", "dhT");
  if (dcT.defined() && dcT.numel() > 0)
    checkLstmArg(dcT, gates, at::kFloat, {B, lstm::kH}, "lstm bwd", "dcT");
  checkLstmArg(whhPackedN, gates, at::kBFloat16, {(int64_t)lstm::kG * lstm::kH}, "lstm bwd",
               "whhPackedN");
  auto opts = gates.options();
  auto fopts = opts.dtype(at::kFloat);
  auto dG = at::empty({T, B, lstm::kG}, opts);
  auto dh0 = at::empty({B, lstm::kH}, opts);
  auto dc0 = at::empty({B, lstm::kH}, fopts);
  int blocks = (B + lstm::kBM - 1) / lstm::kBM;
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(lstm::lstm_bwd_kernel, dim3(blocks), dim3(lstm::kThreads), 0, stream,
                     reinterpret_cast<const lstm::bf16*>(gates.data_ptr()), cs.data_ptr<float>(),
                     c0.data_ptr<float>(), notdone.data_ptr<float>(),
                     reinterpret_cast<const lstm::bf16*>(dH.data_ptr()),
                     (dhT.defined() && dhT.numel() > 0)
                         ? reinterpret_cast<const lstm::bf16*>(dhT.data_ptr())
                         : nullptr,
                     (dcT.defined() && dcT.numel() > 0) ? dcT.data_ptr<float>() : nullptr,
                     reinterpret_cast<const lstm::bf16*>(whhPackedN.data_ptr()),
                     reinterpret_cast<lstm::bf16*>(dG.data_ptr()),
                     reinterpret_cast<lstm::bf16*>(dh0.data_ptr()), dc0.data_ptr<float>(), T, B);
  return {dG, dh0, dc0};
}

std::vector<at::Tensor> vtrace_from_log_rhos(at::Tensor log_rhos, at::Tensor discounts,
                                             at::Tensor rewards, at::Tensor values,
                                             at::Tensor bootstrap, double rho_bar,
                                             double pg_rho_bar) {
  TORCH_CHECK(log_rhos.is_cuda() && log_rhos.dtype() == at::kFloat, "vtrace: float32 CUDA input");
  TORCH_CHECK(log_rhos.dim() == 2, "vtrace: [T,B] expected");
  int T = log_rhos.size(0);
  int B = log_rhos.size(1);
  auto vs = at::empty_like(values);
  auto pg = at::empty_like(values);
  int threads = 256;
  int blocks = (B + threads - 1) / threads;
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(vtrace_scan_kernel, dim3(blocks), dim3(threads), 0, stream,
                     log_rhos.data_ptr<float>(), discounts.data_ptr<float>(),
                     rewards.data_ptr<float>(), values.data_ptr<float>(),
                     bootstrap.data_ptr<float>(), vs.data_ptr<float>(), pg.data_ptr<float>(), T,
                     B, (float)rho_bar, (float)pg_rho_bar);
  return {vs, pg};
}

std::vector<at::Tensor> impala_loss(at::Tensor logits, at::Tensor actions,
                                    at::Tensor pg_advantages, at::Tensor vs, at::Tensor baseline,
                                    double entropy_cost, double baseline_cost,
                                    double grad_scale) {
  TORCH_CHECK(logits.is_cuda() && logits.dtype() == at::kFloat, "loss: float32 CUDA input");
  auto lc = logits.contiguous();
  auto ac = actions.contiguous();
  auto pc = pg_advantages.contiguous();
  auto vc = vs.contiguous();
  auto bc = baseline.contiguous();
  TORCH_CHECK(lc.dim() >= 1 && lc.numel() > 0, "loss: non-empty [..., A] logits expected");
  int64_t A = lc.size(-1);
  int64_t N = lc.numel() / A;
  // the kernel reads one element of each per-row operand for every row
  auto checkRows = [&](const at::Tensor& t, at::ScalarType dtype, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == lc.device() && t.scalar_type() == dtype,
                "loss: ", name, " must be a ", dtype, " tensor on the logits' device");
    TORCH_CHECK(t.numel() == N, "loss: ", name, " has ", t.numel(), " elements, expected ", N);
  };
  checkRows(ac, at::kLong, "actions");
  checkRows(pc, at::kFloat, "pg_advantages");
  checkRows(vc, at::kFloat, "vs");
  checkRows(bc, at::kFloat, "baseline");
  auto grad_logits = at::empty_like(lc);
  auto grad_baseline = at::empty_like(bc);
  auto loss_parts = at::zeros({3}, lc.options());
  int wavesPerBlock = 4;
  int threads = kWave * wavesPerBlock;
  int blocks = (N + wavesPerBlock - 1) / wavesPerBlock;
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(impala_loss_kernel, dim3(blocks), dim3(threads), 0, stream,
                     lc.data_ptr<float>(), ac.data_ptr<int64_t>(), pc.data_ptr<float>(),
                     vc.data_ptr<float>(), bc.data_ptr<float>(), grad_logits.data_ptr<float>(),
                     grad_baseline.data_ptr<float>(), loss_parts.data_ptr<float>(), (int)N,
                     (int)A, (float)entropy_cost, (float)baseline_cost, (float)grad_scale);
  return {loss_parts, grad_logits, grad_baseline};
}

// Pin an existing CPU range (e.g. the EnvPool shared-memory segment) so
// tensor views into it qualify for async H2D DMA.
void register_host_memory(at::Tensor t) {
  TORCH_CHECK(t.device().is_cpu(), "register_host_memory: CPU tensor expected");
  hipError_t err = hipHostRegister(t.data_ptr(), t.nbytes(), hipHostRegisterDefault);
  if (err == hipErrorHostMemoryAlreadyRegistered) {
    (void)hipGetLastError();
    return;
  }
  TORCH_CHECK(err == hipSuccess, "hipHostRegister failed: ", hipGetErrorString(err));
}

at::Tensor frames_u8_to_bf16_nhwc(at::Tensor x, double scale, int64_t padChannels) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.dtype() == at::kByte,
              "frames: 4D uint8 CUDA tensor expected");
  auto xc = x.contiguous();
  int N = xc.size(0), C = xc.size(1), H = xc.size(2), W = xc.size(3);
  const int CO = padChannels > C ? (int)padChannels : C;
  auto out = at::empty({N, CO, H, W},
                       xc.options().dtype(at::kBFloat16).memory_format(at::MemoryFormat::ChannelsLast));
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  int threads = 256;
  if (CO == 8 && C <= 8) {
    int64_t total = (int64_t)N * H * W;
    int64_t blocks = (total + threads - 1) / threads;
    hipLaunchKernelGGL(frames_u8_pad8_kernel, dim3(blocks), dim3(threads), 0, stream,
                       xc.data_ptr<uint8_t>(), reinterpret_cast<__bf16*>(out.data_ptr()),
                       (float)scale, N, C, (int64_t)H * W);
    return out;
  }
  int64_t total = (int64_t)N * CO * H * W;
  int64_t blocks = (total + threads - 1) / threads;
  hipLaunchKernelGGL(frames_u8_to_bf16_nhwc_kernel, dim3(blocks), dim3(threads), 0, stream,
                     xc.data_ptr<uint8_t>(),
                     reinterpret_cast<hip_bfloat16*>(out.data_ptr()), (float)scale, N, C, H, W,
                     CO);
  return out;
}

at::Tensor conv1_u8_nhwc(at::Tensor x, at::Tensor w, at::Tensor bias, double scale) {
  TORCH_CHECK(x.is_cuda() && x.dtype() == at::kByte && x.dim() == 4 && x.size(1) == 4,
              "conv1: uint8 [N,4,H,W] expected");
  TORCH_CHECK(w.dtype() == at::kBFloat16 && w.numel() == 3 * 3 * 4 * 16,
              "conv1: packed bf16 [3,3,4,16] weights expected");
  auto xc = x.contiguous();
  int N = xc.size(0), H = xc.size(2), W = xc.size(3);
  auto out = at::empty({N, 16, H, W},
                       xc.options().dtype(at::kBFloat16).memory_format(at::MemoryFormat::ChannelsLast));
  int64_t total = (int64_t)N * H * ((W + 1) / 2);  // 2 output pixels/thread
  int threads = 256;
  int64_t blocks = (total + threads - 1) / threads;
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(conv1_u8_nhwc_kernel, dim3(blocks), dim3(threads), 0, stream,
                     xc.data_ptr<uint8_t>(),
                     reinterpret_cast<const hip_bfloat16*>(w.contiguous().data_ptr()),
                     reinterpret_cast<const hip_bfloat16*>(bias.contiguous().data_ptr()),
                     reinterpret_cast<hip_bfloat16*>(out.data_ptr()), (float)scale, N, H, W);
  return out;
}

std::vector<at::Tensor> maxpool3x3s2_fwd(at::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, "maxpool: 4D CUDA tensor expected");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast), "maxpool: channels_last expected");
  int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  int OH = (H + 1) / 2, OW = (W + 1) / 2;
  auto out = at::empty({N, C, OH, OW}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  auto idx = at::empty({N, C, OH, OW},
                       x.options().dtype(at::kByte).memory_format(at::MemoryFormat::ChannelsLast));
  TORCH_CHECK(C % 8 == 0, "maxpool: channels must be a multiple of 8");
  int64_t total = (int64_t)N * OH * OW * (C / 8);
  int threads = 256;
  int64_t blocks = (total + threads - 1) / threads;
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::kBFloat16, at::kHalf, x.scalar_type(), "maxpool3x3s2_fwd", [&] {
        hipLaunchKernelGGL(maxpool3x3s2_fwd_kernel<scalar_t>, dim3(blocks), dim3(threads), 0,
                           stream, x.data_ptr<scalar_t>(), out.data_ptr<scalar_t>(),
                           idx.data_ptr<uint8_t>(), N, H, W, C, OH, OW);
      });
  return {out, idx};
}

at::Tensor maxpool3x3s2_bwd(at::Tensor gout, at::Tensor idx, int64_t H, int64_t W) {
  TORCH_CHECK(gout.is_cuda() && gout.dim() == 4, "maxpool bwd: 4D CUDA tensor expected");
  auto g = gout.contiguous(at::MemoryFormat::ChannelsLast);
  int N = g.size(0), C = g.size(1), OH = g.size(2), OW = g.size(3);
  auto gin = at::empty({N, C, H, W}, g.options().memory_format(at::MemoryFormat::ChannelsLast));
  TORCH_CHECK(C % 8 == 0, "maxpool bwd: channels must be a multiple of 8");
  int64_t total = (int64_t)N * H * W * (C / 8);
  int threads = 256;
  int64_t blocks = (total + threads - 1) / threads;
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::kBFloat16, at::kHalf, g.scalar_type(), "maxpool3x3s2_bwd", [&] {
        hipLaunchKernelGGL(maxpool3x3s2_bwd_kernel<scalar_t>, dim3(blocks), dim3(threads), 0,
                           stream, g.data_ptr<scalar_t>(), idx.data_ptr<uint8_t>(),
                           gin.data_ptr<scalar_t>(), N, (int)H, (int)W, C, OH, OW);
      });
  return gin;
}

// ------------------------- fused conv-bias epilogues -----------------------
// MIOpen applies conv bias as its own full-tensor pass (SubTensorOpWithScalar
// in the kernel trace) and torch's relu / residual add are two more passes
// over HBM. Running the convs bias-free (F.conv2d(..., None)) and folding the
// bias into the next elementwise op turns (bias, relu) and (bias, add) into
// ONE bandwidth-bound pass each. Per-channel bias commutes with the
// per-channel spatial maxpool, so a section conv's bias rides through the
// pool into the next block's bias_relu and the residual shortcut (the second
// bias of bias_add2). Model integration: moolib_amd/models/atari.py
// (reference architecture examples/atari/models.py:9-153 is unchanged
// mathematically).

template <typename T>
__global__ void bias_relu_fwd_kernel(const T* __restrict__ x, const T* __restrict__ b,
                                     T* __restrict__ y, int64_t total8, int c8n) {
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= total8) return;
  int c8 = tid % c8n;
  const Vec8<T> vx = *reinterpret_cast<const Vec8<T>*>(x + tid * 8);
  const Vec8<T> vb = *reinterpret_cast<const Vec8<T>*>(b + (int64_t)c8 * 8);
  Vec8<T> vy;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = (float)vx.v[j] + (float)vb.v[j];
    vy.v[j] = (T)(v > 0.f ? v : 0.f);
  }
  *reinterpret_cast<Vec8<T>*>(y + tid * 8) = vy;
}

// dx = dy * (y > 0); db reduced without contention: a grid-stride loop with
// stride = blockDim*gridDim accumulates db partials in registers, then one
// LDS pass and one global atomic per channel per workgroup. Each thread's
// channel group is FIXED at tid0 % c8n, which is only right if the stride is
// a multiple of c8n: blockDim (256) covers c8n's power-of-two part and the
// host rounds gridDim to a multiple of its odd part whenever the loop
// iterates (channelSumBlocks). The naive
// one-atomic-per-element version serialized 256 threads onto C addresses
// and ran 14x slower than bandwidth.
template <typename T>
__global__ void bias_relu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y,
                                     T* __restrict__ dx, float* __restrict__ db,
                                     int64_t total8, int c8n) {
  __shared__ float lds_db[64];
  int C = c8n * 8;
  if (threadIdx.x < C) lds_db[threadIdx.x] = 0.f;
  __syncthreads();
  // a multiple of c8n: blockDim (256) is a multiple of c8n's power-of-two
  // part, gridDim of its odd part (channelSumBlocks on the host)
  int64_t stride = (int64_t)blockDim.x * gridDim.x;
  int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int c8 = (int)(tid0 % c8n);
  for (int64_t tid = tid0; tid < total8; tid += stride) {
    const Vec8<T> vdy = *reinterpret_cast<const Vec8<T>*>(dy + tid * 8);
    const Vec8<T> vy = *reinterpret_cast<const Vec8<T>*>(y + tid * 8);
    Vec8<T> vdx;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float g = (float)vy.v[j] > 0.f ? (float)vdy.v[j] : 0.f;
      vdx.v[j] = (T)g;
      acc[j] += g;
    }
    *reinterpret_cast<Vec8<T>*>(dx + tid * 8) = vdx;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) atomicAdd(&lds_db[c8 * 8 + j], acc[j]);
  __syncthreads();
  if (threadIdx.x < C) atomicAdd(&db[threadIdx.x], lds_db[threadIdx.x]);
}

// Per-channel sum of an NHWC tensor (bias gradients): same small-grid +
// LDS + one-global-atomic-per-channel layout as bias_relu_bwd_kernel.
// aten's bf16 reduce runs this shape at ~0.4 TB/s (22.5 us at
// [672,32,21,21], profiles/evidence/r3i_learnprof.txt).
template <typename T>
__global__ void channel_sum_kernel(const T* __restrict__ x, float* __restrict__ out,
                                   int64_t total8, int c8n) {
  __shared__ float lds[64];
  int C = c8n * 8;
  if (threadIdx.x < C) lds[threadIdx.x] = 0.f;
  __syncthreads();
  // a multiple of c8n: blockDim (256) is a multiple of c8n's power-of-two
  // part, gridDim of its odd part (channelSumBlocks on the host)
  int64_t stride = (int64_t)blockDim.x * gridDim.x;
  int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int c8 = (int)(tid0 % c8n);
  for (int64_t tid = tid0; tid < total8; tid += stride) {
    const Vec8<T> v = *reinterpret_cast<const Vec8<T>*>(x + tid * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += (float)v.v[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) atomicAdd(&lds[c8 * 8 + j], acc[j]);
  __syncthreads();
  if (threadIdx.x < C) atomicAdd(&out[threadIdx.x], lds[threadIdx.x]);
}

// y = x + b1 + s (+ b2): residual close with the producing conv's bias and,
// when the shortcut came through a pooled bias-free section conv, that
// conv's pending bias too.
template <typename T>
__global__ void bias_add2_fwd_kernel(const T* __restrict__ x, const T* __restrict__ b1,
                                     const T* __restrict__ s, const T* __restrict__ b2,
                                     T* __restrict__ y, int64_t total8, int c8n) {
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= total8) return;
  int c8 = tid % c8n;
  const Vec8<T> vx = *reinterpret_cast<const Vec8<T>*>(x + tid * 8);
  const Vec8<T> vs = *reinterpret_cast<const Vec8<T>*>(s + tid * 8);
  const Vec8<T> vb1 = *reinterpret_cast<const Vec8<T>*>(b1 + (int64_t)c8 * 8);
  Vec8<T> vy;
  if (b2 != nullptr) {
    const Vec8<T> vb2 = *reinterpret_cast<const Vec8<T>*>(b2 + (int64_t)c8 * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      vy.v[j] = (T)((float)vx.v[j] + (float)vb1.v[j] + (float)vs.v[j] + (float)vb2.v[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      vy.v[j] = (T)((float)vx.v[j] + (float)vb1.v[j] + (float)vs.v[j]);
  }
  *reinterpret_cast<Vec8<T>*>(y + tid * 8) = vy;
}

static void checkNhwcPair(const at::Tensor& x, const char* who) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, who, ": 4D CUDA tensor expected");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast), who, ": channels_last expected");
  TORCH_CHECK(x.size(1) % 8 == 0, who, ": channels must be a multiple of 8");
}

// Grid size for the two channel-sum kernels (256 threads). Their threads keep
// the channel octet tid0 % c8n for the whole grid-stride loop, so the stride
// 256*blocks must be a multiple of c8n = C/8 (1..8). 256 covers the
// power-of-two part; when the cap makes the loop iterate, blocks is rounded
// down to a multiple of c8n's odd part (3, 5 or 7 for C = 24/48, 40, 56).
// C = 16 and 32 have odd part 1: their launch geometry is untouched.
static int64_t channelSumBlocks(int64_t total8, int threads, int64_t blockCap, int c8n) {
  int64_t blocks = std::min<int64_t>((total8 + threads - 1) / threads, blockCap);
  int64_t odd = c8n;
  while (odd % 2 == 0) odd /= 2;
  if (blocks * threads < total8) blocks = std::max<int64_t>(blocks / odd, 1) * odd;
  return blocks;
}

at::Tensor bias_relu_fwd(at::Tensor x, at::Tensor b) {
  checkNhwcPair(x, "bias_relu");
  int C = x.size(1);
  TORCH_CHECK(b.numel() == C && b.scalar_type() == x.scalar_type(), "bias_relu: bad bias");
  auto out = at::empty_like(x, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  int64_t total8 = x.numel() / 8;
  int threads = 256;
  int64_t blocks = (total8 + threads - 1) / threads;
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::kBFloat16, at::kHalf, x.scalar_type(), "bias_relu_fwd", [&] {
        hipLaunchKernelGGL(bias_relu_fwd_kernel<scalar_t>, dim3(blocks), dim3(threads), 0, stream,
                           x.data_ptr<scalar_t>(), b.contiguous().data_ptr<scalar_t>(),
                           out.data_ptr<scalar_t>(), total8, C / 8);
      });
  return out;
}

std::vector<at::Tensor> bias_relu_bwd(at::Tensor dy, at::Tensor y) {
  checkNhwcPair(y, "bias_relu_bwd");
  TORCH_CHECK(dy.is_cuda() && dy.sizes() == y.sizes() && dy.scalar_type() == y.scalar_type(),
              "bias_relu_bwd: dy must match y in device, shape and dtype");
  auto g = dy.contiguous(at::MemoryFormat::ChannelsLast);
  int C = y.size(1);
  TORCH_CHECK(C <= 64, "bias_relu_bwd: C <= 64 (LDS accumulator)");
  auto dx = at::empty_like(y, y.options().memory_format(at::MemoryFormat::ChannelsLast));
  auto db = at::zeros({C}, y.options().dtype(at::kFloat));
  int64_t total8 = y.numel() / 8;
  int threads = 256;
  // grid-stride with a SMALL grid: each block ends with one global atomic
  // per channel, so the per-block finalization atomics — not occupancy —
  // set the floor. Swept caps 256..8192 at the three learner shapes
  // (profiles/evidence/r4{i,j}_bias_micro.txt): per-shape optima
  // 768/384/256 fit blocks = clamp(total8/3000, 256, 768), 29-51% faster
  // than the old 2048 cap. MOOLIB_AMD_BIAS_BWD_BLOCKS overrides for A/Bs.
  static const int64_t blockCapEnv = []() {
    const char* s = std::getenv("MOOLIB_AMD_BIAS_BWD_BLOCKS");
    return s ? std::strtoll(s, nullptr, 10) : (int64_t)0;
  }();
  int64_t blockCap = blockCapEnv > 0
                         ? blockCapEnv
                         : std::min<int64_t>(std::max<int64_t>(total8 / 3000, 256), 768);
  int64_t blocks = channelSumBlocks(total8, threads, blockCap, C / 8);
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::kBFloat16, at::kHalf, y.scalar_type(), "bias_relu_bwd", [&] {
        hipLaunchKernelGGL(bias_relu_bwd_kernel<scalar_t>, dim3(blocks), dim3(threads), 0, stream,
                           g.data_ptr<scalar_t>(), y.data_ptr<scalar_t>(),
                           dx.data_ptr<scalar_t>(), db.data_ptr<float>(), total8, C / 8);
      });
  return {dx, db};
}

at::Tensor channel_sum_fp32(at::Tensor x) {
  checkNhwcPair(x, "channel_sum");
  int C = x.size(1);
  TORCH_CHECK(C <= 64, "channel_sum: C <= 64 (LDS accumulator)");
  auto out = at::zeros({C}, x.options().dtype(at::kFloat));
  int64_t total8 = x.numel() / 8;
  int threads = 256;
  // small grid: the per-block channel atomics set the floor (see
  // bias_relu_bwd above; same sweep, profiles/evidence/r4j_bias_micro.txt)
  int64_t blockCap = std::min<int64_t>(std::max<int64_t>(total8 / 3000, 256), 768);
  int64_t blocks = channelSumBlocks(total8, threads, blockCap, C / 8);
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::kBFloat16, at::kHalf, x.scalar_type(), "channel_sum", [&] {
        hipLaunchKernelGGL(channel_sum_kernel<scalar_t>, dim3(blocks), dim3(threads), 0, stream,
                           x.data_ptr<scalar_t>(), out.data_ptr<float>(), total8, C / 8);
      });
  return out;
}

at::Tensor bias_add2_fwd(at::Tensor x, at::Tensor b1, at::Tensor s,
                         c10::optional<at::Tensor> b2) {
  checkNhwcPair(x, "bias_add2");
  checkNhwcPair(s, "bias_add2(shortcut)");
  int C = x.size(1);
  TORCH_CHECK(b1.numel() == C && b1.scalar_type() == x.scalar_type(), "bias_add2: bad bias1");
  at::Tensor b2c;
  if (b2.has_value()) {
    TORCH_CHECK(b2->numel() == C && b2->scalar_type() == x.scalar_type(), "bias_add2: bad bias2");
    b2c = b2->contiguous();
  }
  auto out = at::empty_like(x, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  int64_t total8 = x.numel() / 8;
  int threads = 256;
  int64_t blocks = (total8 + threads - 1) / threads;
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::kBFloat16, at::kHalf, x.scalar_type(), "bias_add2_fwd", [&] {
        hipLaunchKernelGGL(bias_add2_fwd_kernel<scalar_t>, dim3(blocks), dim3(threads), 0, stream,
                           x.data_ptr<scalar_t>(), b1.contiguous().data_ptr<scalar_t>(),
                           s.data_ptr<scalar_t>(),
                           b2.has_value() ? b2c.data_ptr<scalar_t>() : nullptr,
                           out.data_ptr<scalar_t>(), total8, C / 8);
      });
  return out;
}

// ------------------------------------------------ batched slice copies
//
// The Batcher (csrc/batcher.cc; reference semantics src/moolib.cc:651-752)
// fills preallocated [T,B,...] targets with one copy_ per nest leaf per
// call — on the IMPALA hot path that is ~8 tiny __amd_rocclr_copyBuffer
// launches per rollout step (~0.7 ms/optimizer step of ramp-dominated
// copies in the r1 profile). This kernel moves every leaf of one
// stack()/cat() call in a single launch: each entry is a strided
// rows x rowBytes region, the descriptor table travels in the kernel-arg
// block (no H2D staging), and blockIdx.y picks the entry so the per-entry
// vector width is wave-uniform.

struct CopyDesc {
  const uint8_t* src;
  uint8_t* dst;
  int64_t rows;
  int64_t rowBytes;
  int64_t srcStrideB;  // bytes between rows
  int64_t dstStrideB;
  int32_t vec;  // 16 / 4 / 1: granularity valid for ptrs, strides, rowBytes
  int32_t pad;
};

constexpr int kMaxCopyDescs = 24;  // 24 * 56 B comfortably under the 4 KB arg limit
struct CopyDescPack {
  CopyDesc d[kMaxCopyDescs];
  int32_t n;
};

template <typename V>
DEV_INLINE void copyRun(const CopyDesc& e, int64_t start, int64_t step, int64_t total) {
  for (int64_t idx = start; idx < total; idx += step) {
    int64_t byte = idx * (int64_t)sizeof(V);
    int64_t row = byte / e.rowBytes;
    int64_t col = byte - row * e.rowBytes;
    *reinterpret_cast<V*>(e.dst + row * e.dstStrideB + col) =
        *reinterpret_cast<const V*>(e.src + row * e.srcStrideB + col);
  }
}

__global__ void batched_copy_kernel(CopyDescPack pack) {
  const CopyDesc& e = pack.d[blockIdx.y];
  int64_t units = e.rows * e.rowBytes / e.vec;
  int64_t start = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t step = (int64_t)gridDim.x * blockDim.x;
  if (e.vec == 16) copyRun<uint4>(e, start, step, units);
  else if (e.vec == 4) copyRun<uint32_t>(e, start, step, units);
  else copyRun<uint8_t>(e, start, step, units);
}

namespace {

// Express a tensor view as rows x contiguous-rowElems with a uniform row
// stride (the shape select()/narrow() of a contiguous buffer produces).
// Returns false for layouts that need a general copy.
bool rowDecompose(const at::Tensor& t, int64_t& rows, int64_t& rowElems, int64_t& strideEl) {
  int64_t inner = 1;
  int d = t.dim() - 1;
  for (; d >= 0; --d) {
    if (t.size(d) == 1) continue;
    if (t.stride(d) != inner) break;
    inner *= t.size(d);
  }
  rowElems = inner;
  if (d < 0) {  // fully contiguous
    rows = 1;
    strideEl = inner;
    return true;
  }
  rows = t.size(d);
  strideEl = t.stride(d);
  for (int i = d - 1; i >= 0; --i) {
    if (t.size(i) == 1) continue;
    if (t.stride(i) != strideEl * rows) return false;
    rows *= t.size(i);
  }
  return strideEl >= rowElems;
}

int vecWidthFor(const void* a, const void* b, int64_t rowBytes, int64_t sA, int64_t sB) {
  auto ok = [&](int64_t v) {
    return ((uintptr_t)a % v == 0) && ((uintptr_t)b % v == 0) && (rowBytes % v == 0) &&
           (sA % v == 0) && (sB % v == 0);
  };
  if (ok(16)) return 16;
  if (ok(4)) return 4;
  return 1;
}

}  // namespace

// dsts[i] <- srcs[i] for same-shaped same-dtype CUDA pairs, all in one
// launch (chunked by kMaxCopyDescs). Pairs this kernel can't express
// (cross-device, CPU, exotic strides) fall back to copy_ individually, so
// the call is semantically total.
void batched_copy(std::vector<at::Tensor> dsts, std::vector<at::Tensor> srcs) {
  TORCH_CHECK(dsts.size() == srcs.size(), "batched_copy: length mismatch");
  CopyDescPack pack;
  pack.n = 0;
  int64_t maxUnits = 0;
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  auto flush = [&]() {
    if (pack.n == 0) return;
    int threads = 256;
    int64_t blocksX = std::min<int64_t>((maxUnits + threads - 1) / threads, 1024);
    hipLaunchKernelGGL(batched_copy_kernel, dim3(blocksX, pack.n), dim3(threads), 0, stream,
                       pack);
    pack.n = 0;
    maxUnits = 0;
  };
  for (size_t i = 0; i < dsts.size(); ++i) {
    at::Tensor& dst = dsts[i];
    at::Tensor& src = srcs[i];
    bool fused = false;
    if (dst.is_cuda() && src.is_cuda() && dst.device() == src.device() &&
        dst.scalar_type() == src.scalar_type() && dst.numel() == src.numel() &&
        dst.numel() > 0) {
      int64_t dRows, dRowEl, dStride, sRows, sRowEl, sStride;
      if (rowDecompose(dst, dRows, dRowEl, dStride) &&
          rowDecompose(src, sRows, sRowEl, sStride)) {
        // Unify row shapes: a fully contiguous side adopts the other's rows.
        if (dRows == 1 && sRows > 1) {
          dRows = sRows;
          dRowEl = sRowEl;
          dStride = sRowEl;
        } else if (sRows == 1 && dRows > 1) {
          sRows = dRows;
          sRowEl = dRowEl;
          sStride = dRowEl;
        }
        if (dRows == sRows && dRowEl == sRowEl) {
          int64_t esize = dst.element_size();
          CopyDesc e;
          e.src = (const uint8_t*)src.data_ptr();
          e.dst = (uint8_t*)dst.data_ptr();
          e.rows = dRows;
          e.rowBytes = dRowEl * esize;
          e.srcStrideB = sStride * esize;
          e.dstStrideB = dStride * esize;
          e.vec = vecWidthFor(e.src, e.dst, e.rowBytes, e.srcStrideB, e.dstStrideB);
          pack.d[pack.n++] = e;
          maxUnits = std::max(maxUnits, e.rows * e.rowBytes / e.vec);
          if (pack.n == kMaxCopyDescs) flush();
          fused = true;
        }
      }
    }
    if (!fused) dst.copy_(src, /*non_blocking=*/true);
  }
  flush();
}

// Device-side prioritized replay (sum tree + indexed row gather/scatter);
// uses kMaxCopyDescs above.
#include "replay.hip.inc"

// Fused actor head: Philox categorical sampling and epsilon-greedy dueling Q.
#include "act.hip.inc"

// Fused flat Adam step: grad norm, clip, update and bf16 shadow in two launches.
#include "optim.hip.inc"

// ------------------------------------------- batched conv-weight repack
//
// The conv3x3 path keeps per-conv MFMA-packed weight buffers (fwd pack +
// dgrad pack) that must refresh once per optimizer step. Doing that with
// torch ops is ~14 kernels per conv per direction (flip/permute/cat/
// contiguous) replayed inside the captured optimizer graph (~0.4 ms and
// ~200 launches per step in the r2 profile); this kernel rewrites EVERY
// pack in one launch: each output element decodes its (ct, kk, lane, e)
// fragment coordinate and reads the one weight element it mirrors.
// Layouts mirror ops/lstm.py pack_mfma_b and ops/conv3x3.py
// pack_weight/pack_weight_dgrad exactly (tested against them).

namespace repack3x3 {

using bf16 = __bf16;

struct Desc {
  const bf16* w;  // [K, C, 3, 3], arbitrary strides (channels_last safe)
  bf16* outF;     // fwd pack, ceil(9*Cp/32)*32*K elems, or null
  bf16* outD;     // dgrad pack, ceil(9K/32)*32*C elems, or null
  int64_t sK, sC, sH, sW;  // element strides of w
  int32_t C, K;
  int32_t Cp;     // fwd pack channel count (>= C; channels C..Cp are zero —
                  // the C=4 first conv packs as C=8 for the MFMA template)
};
constexpr int kMaxDescs = 20;
struct Pack {
  Desc d[kMaxDescs];
  int32_t n;
};

__global__ void repack3x3_kernel(Pack pack) {
  const Desc& d = pack.d[blockIdx.y];
  const int KKf = (9 * d.Cp + 31) / 32;
  const int KKd = (9 * d.K + 31) / 32;
  const int nF = d.outF ? KKf * 32 * d.K : 0;
  const int nD = d.outD ? KKd * 32 * d.C : 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nF + nD;
       i += gridDim.x * blockDim.x) {
    const bool isF = i < nF;
    const int idx = isF ? i : i - nF;
    const int KK = isF ? KKf : KKd;
    const int CC = isF ? d.Cp : d.K;  // in-channels of this direction
    // idx = ((ct*KK + kk)*64 + lane)*8 + e
    const int e = idx & 7;
    const int lane = (idx >> 3) & 63;
    const int rest = idx >> 9;
    const int kk = rest % KK;
    const int ct = rest / KK;
    const int kd = kk * 32 + (lane >> 4) * 8 + e;
    const int n = ct * 16 + (lane & 15);
    bf16 v = (bf16)0.f;
    if (kd < 9 * CC) {
      const int tap = kd / CC, c = kd % CC;
      const int kh = tap / 3, kw = tap % 3;
      if (isF) {
        if (c < d.C) v = d.w[n * d.sK + c * d.sC + kh * d.sH + kw * d.sW];
      } else {
        // dgrad: W'[c_out=n... ] = w[c][n][2-kh][2-kw]
        v = d.w[c * d.sK + n * d.sC + (2 - kh) * d.sH + (2 - kw) * d.sW];
      }
    }
    (isF ? d.outF : d.outD)[idx] = v;
  }
}

}  // namespace repack3x3

// Refresh fwd/dgrad MFMA packs for a batch of convs in ONE launch.
// dgrad entries may be empty tensors (conv1 has no dgrad pack).
void repack3x3_batched(std::vector<at::Tensor> ws, std::vector<at::Tensor> fwdBufs,
                       std::vector<at::Tensor> dgradBufs, std::vector<int64_t> packChannels) {
  TORCH_CHECK(ws.size() == fwdBufs.size() && ws.size() == dgradBufs.size() &&
                  ws.size() == packChannels.size(),
              "repack3x3: list length mismatch");
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  repack3x3::Pack pack;
  pack.n = 0;
  auto flush = [&]() {
    if (pack.n == 0) return;
    hipLaunchKernelGGL(repack3x3::repack3x3_kernel, dim3(32, pack.n), dim3(256), 0, stream,
                       pack);
    pack.n = 0;
  };
  for (size_t i = 0; i < ws.size(); ++i) {
    at::Tensor& w = ws[i];
    TORCH_CHECK(w.is_cuda() && w.dim() == 4 && w.scalar_type() == at::kBFloat16,
                "repack3x3: bf16 4D CUDA weight expected");
    const int K = w.size(0), C = w.size(1);
    repack3x3::Desc e;
    e.w = reinterpret_cast<const repack3x3::bf16*>(w.data_ptr());
    e.sK = w.stride(0);
    e.sC = w.stride(1);
    e.sH = w.stride(2);
    e.sW = w.stride(3);
    e.C = C;
    e.K = K;
    e.Cp = packChannels[i] > C ? (int)packChannels[i] : C;
    e.outF = nullptr;
    e.outD = nullptr;
    if (fwdBufs[i].defined() && fwdBufs[i].numel() > 0) {
      TORCH_CHECK(fwdBufs[i].numel() == (9 * e.Cp + 31) / 32 * 32 * K, "repack3x3: fwd size");
      e.outF = reinterpret_cast<repack3x3::bf16*>(fwdBufs[i].data_ptr());
    }
    if (dgradBufs[i].defined() && dgradBufs[i].numel() > 0) {
      TORCH_CHECK(dgradBufs[i].numel() == (9 * K + 31) / 32 * 32 * C, "repack3x3: dgrad size");
      e.outD = reinterpret_cast<repack3x3::bf16*>(dgradBufs[i].data_ptr());
    }
    pack.d[pack.n++] = e;
    if (pack.n == repack3x3::kMaxDescs) flush();
  }
  flush();
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "moolib_amd gfx950 HIP kernels";
  m.def("register_host_memory", &register_host_memory);
  m.def("repack3x3_batched", &repack3x3_batched,
        "refresh all conv MFMA weight packs (fwd + dgrad) in one launch");
  m.def("batched_copy", &batched_copy,
        "copy many (dst<-src) slice pairs in one kernel launch (gfx950)");
  m.def("maxpool3x3s2_fwd", &maxpool3x3s2_fwd, "NHWC 3x3/2 maxpool forward (gfx950)");
  m.def("maxpool3x3s2_bwd", &maxpool3x3s2_bwd, "NHWC 3x3/2 maxpool backward (gather, no atomics)");
  m.def("bias_relu_fwd", &bias_relu_fwd, "fused conv-bias + relu, one NHWC pass (gfx950)");
  m.def("bias_relu_bwd", &bias_relu_bwd, "bias_relu backward: dx + fp32 db in one pass");
  m.def("bias_add2_fwd", &bias_add2_fwd, "fused residual close: x + bias1 + shortcut (+ bias2)");
  m.def("channel_sum_fp32", &channel_sum_fp32,
        "NHWC per-channel fp32 sum (bias gradients; small-grid atomics)");
  m.def("frames_u8_to_bf16_nhwc", &frames_u8_to_bf16_nhwc,
        "fused uint8->bf16 NHWC scale (optionally zero-padding channels)",
        py::arg("x"), py::arg("scale"), py::arg("pad_channels") = 0);
  m.def("conv1_u8_nhwc", &conv1_u8_nhwc, "fused uint8 frames -> conv(4->16,3x3)+bias, NHWC bf16");
  m.def("conv3x3_nhwc_fused", &conv3x3_nhwc_fused,
        "MFMA 3x3/s1/p1 NHWC conv with fused relu/bias prologue + bias/relu/residual epilogue",
        py::arg("x"), py::arg("w_packed"), py::arg("k"), py::arg("relu_in") = false,
        py::arg("bias_in") = py::none(), py::arg("epi") = 0, py::arg("bias1") = py::none(),
        py::arg("res") = py::none(), py::arg("bias2") = py::none(), py::arg("rt") = 0);
  m.def("wgrad3x3_nhwc", &wgrad3x3_nhwc,
        "3x3/s1/p1 conv weight gradient on MFMA (row-slab LDS staging, gfx950)");
  m.def("lstm_fused_fwd", &lstm_fused_fwd, "fused masked LSTM sequence scan fwd (MFMA, gfx950)");
  m.def("lstm_fused_bwd", &lstm_fused_bwd, "fused masked LSTM sequence scan bwd (MFMA, gfx950)");
  m.def("vtrace_from_log_rhos", &vtrace_from_log_rhos, "fused V-trace scan (gfx950)");
  m.def("impala_loss", &impala_loss, "fused IMPALA loss fwd+grad (gfx950)");
  m.def("r2d2_loss", &r2d2_loss,
        "fused R2D2 loss: n-step double-Q TD errors, sequence loss, priorities, grad_q (gfx950)",
        py::arg("q"), py::arg("q_target"), py::arg("actions"), py::arg("rewards"),
        py::arg("discounts"), py::arg("mask"), py::arg("is_weights"), py::arg("n"),
        py::arg("eps"), py::arg("rescale"), py::arg("eta"), py::arg("grad_scale"),
        py::arg("grad_out") = py::none());
  m.def("r2d2_actor_priority", &r2d2_actor_priority,
        "initial sequence priorities [K] and TD errors [T,K] from an actor's q_taken / q_max, "
        "reward and done in the actor's layout; one launch (gfx950)",
        py::arg("q_taken"), py::arg("q_max"), py::arg("reward"), py::arg("done"), py::arg("n"),
        py::arg("discount"), py::arg("eps"), py::arg("rescale"), py::arg("eta"),
        py::arg("burn_in"), py::arg("priority_out") = py::none(),
        py::arg("td_out") = py::none());
  m.attr("R2D2_MAX_T") = r2d2::kMaxT;  // longest sequence the r2d2 kernels accept
  m.def("replay_tree_update", &replay_tree_update,
        "sum-tree leaves <- priority^alpha (last wins), ancestors, max_priority (gfx950)",
        py::arg("tree"), py::arg("max_priority"), py::arg("slots"), py::arg("priorities"),
        py::arg("alpha"), py::arg("L"));
  m.def("replay_tree_sample", &replay_tree_sample,
        "stratified sum-tree sample: idx [B], normalised importance weights [B] (gfx950)",
        py::arg("tree"), py::arg("L"), py::arg("size"), py::arg("u"), py::arg("beta"),
        py::arg("idx_out") = py::none(), py::arg("weights_out") = py::none());
  m.def("replay_rows", &replay_rows,
        "gather / scatter whole items of every nest leaf by a device index, one launch",
        py::arg("storage"), py::arg("other"), py::arg("index"), py::arg("mode"));
  m.attr("REPLAY_MAX_UPDATE") = replay::kMaxUpdate;  // slots per replay_tree_update launch
  m.attr("REPLAY_MAX_SAMPLE") = replay::kMaxSample;  // largest replay_tree_sample batch
  m.def("act_categorical", &act_categorical,
        "action ~ softmax(logits) from [seed, step] Philox state or explicit uniforms (gfx950)",
        py::arg("logits"), py::arg("state") = py::none(), py::arg("u") = py::none(),
        py::arg("action_out") = py::none());
  m.def("act_eps_greedy", &act_eps_greedy,
        "epsilon-greedy dueling head: action, q_taken, q_max in one launch (gfx950)",
        py::arg("value"), py::arg("advantage"), py::arg("epsilon"), py::arg("state") = py::none(),
        py::arg("u") = py::none(), py::arg("action_out") = py::none(),
        py::arg("q_taken_out") = py::none(), py::arg("q_max_out") = py::none());
  m.attr("ACT_MAX_ACTIONS") = act::kMaxActions;  // widest row the act kernels accept
  m.def("flat_adam_step", &flat_adam_step,
        "fused flat Adam: grad norm, clip, update of p/m/v, bf16 shadow; two launches (gfx950)",
        py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("shadow"),
        py::arg("step"), py::arg("step_next"), py::arg("lr"), py::arg("partial"),
        py::arg("norm_out"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("max_norm") = py::none());
  m.attr("FLAT_ADAM_MAX_BLOCKS") = optim::kMaxBlocks;        // grid cap, length of `partial`
  m.attr("FLAT_ADAM_PASS_ELEMENTS") = optim::kPassElements;  // elements one grid pass covers
}
