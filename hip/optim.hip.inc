// Fused flat Adam step for gfx950 — included by kernels.hip.
//
// Gradient norm, clip coefficient, Adam update and the bf16 shadow weights of
// ALL parameters in two launches over flat contiguous buffers (the layout of
// flatten_master_shadow). The eager chain it replaces is clip_grad_norm_ (a
// foreach norm, a stack, a norm, a clamp, a foreach mul), about a dozen
// multi-tensor Adam launches and a flat cast-copy; the work itself is one
// memory-bound pass of ~30 bytes per element.
//
//   flat_sumsq_kernel      partial[block] = sum of (double)g*g over the
//                          block's fixed grid-stride share; block 0 also
//                          writes step_next = step + 1.
//   flat_adam_step_kernel  every block reduces partial[0..G) in the same
//                          fixed order (so all blocks hold the same norm
//                          bit for bit), forms the clip coefficient and the
//                          bias corrections, then updates its quads: float4
//                          loads and stores of p, m, v and one 8-byte store of
//                          four bf16 shadow weights. Block 0 writes the
//                          unclipped norm and step = step_next.
//
// No atomics, no host wait, and G depends on N alone: the result is
// bit-reproducible. The step counter ping-pongs between two device words so
// that no kernel reads and writes the same one; lr is read from a device
// scalar, so a schedule changes nothing that a captured graph has baked in.
//
// The unit of work is a quad (4 consecutive elements); the last quad of an
// N that is no multiple of 4 is handled element by element. One grid pass
// covers kMaxBlocks * kThreads quads.
//
// Numerics (moolib_amd/ops/flat_adam.py holds the definition): per element
// everything is fp32 with IEEE sqrtf and division, fp contraction off, in the
// order of the eager path; the sum of squares and the bias corrections
// 1 - beta^t are formed in double and rounded once.

namespace optim {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 1024;
constexpr int64_t kPassElements = (int64_t)kMaxBlocks * kThreads * 4;

inline int64_t quadsOf(int64_t N) { return (N + 3) / 4; }

// Blocks for N elements: enough for one pass, capped. A function of N alone.
inline int gridBlocks(int64_t N) {
  const int64_t blocks = (quadsOf(N) + kThreads - 1) / kThreads;
  return (int)std::min<int64_t>(std::max<int64_t>(blocks, 1), kMaxBlocks);
}

DEV_INLINE double waveSumF64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  return v;  // lane 0 holds the sum
}

// Sum over the block in a fixed order: lanes by shuffles, then the waves in
// index order by thread 0. Every thread returns the total.
DEV_INLINE double blockSumF64(double v, double* sWave, double* sTotal) {
  const int tid = threadIdx.x;
  v = waveSumF64(v);
  if ((tid & 63) == 0) sWave[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    double s = sWave[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s = s + sWave[w];
    *sTotal = s;
  }
  __syncthreads();
  return *sTotal;
}

__global__ __launch_bounds__(kThreads) void flat_sumsq_kernel(
    const float* __restrict__ g, double* __restrict__ partial,
    const int64_t* __restrict__ step_in, int64_t* __restrict__ step_out, int64_t N) {
#pragma clang fp contract(off)
  __shared__ double sWave[kWaves];
  __shared__ double sTotal;
  const int64_t nquad = (N + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  double acc = 0.0;
  for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < nquad; q += stride) {
    const int64_t i = q * 4;
    if (i + 4 <= N) {
      const float4 x = *reinterpret_cast<const float4*>(g + i);
      acc = acc + (double)x.x * (double)x.x;
      acc = acc + (double)x.y * (double)x.y;
      acc = acc + (double)x.z * (double)x.z;
      acc = acc + (double)x.w * (double)x.w;
    } else {
      for (int64_t j = i; j < N; ++j) {
        const double x = (double)g[j];
        acc = acc + x * x;
      }
    }
  }
  const double total = blockSumF64(acc, sWave, &sTotal);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = total;
    if (blockIdx.x == 0) *step_out = *step_in + 1;
  }
}

// beta^t for an integer t >= 0, by squaring, in double (no libm pow on the
// device: a handful of multiplies, each within half an ulp).
DEV_INLINE double powInt(double b, int64_t t) {
#pragma clang fp contract(off)
  double r = 1.0;
  while (t > 0) {
    if (t & 1) r = r * b;
    b = b * b;
    t >>= 1;
  }
  return r;
}

// Round to nearest even; NaN becomes the quiet NaN torch's cast produces.
DEV_INLINE unsigned bf16Bits(float x) {
  const unsigned u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

struct AdamScalars {
  float coef;      // clip coefficient (1 without clipping)
  float w1;        // 1 - beta1
  float beta2;
  float w2;        // 1 - beta2
  float stepSize;  // lr / (1 - beta1^t)
  float bc2Sqrt;   // sqrt(1 - beta2^t)
  float eps;
};

DEV_INLINE void adamElement(const AdamScalars& s, float g, float& p, float& m, float& v) {
#pragma clang fp contract(off)
  const float gh = g * s.coef;
  m = m + (gh - m) * s.w1;
  const float sq = (s.w2 * gh) * gh;
  v = v * s.beta2 + sq;
  const float denom = sqrtf(v) / s.bc2Sqrt + s.eps;
  p = p - (s.stepSize * m) / denom;
}

__global__ __launch_bounds__(kThreads) void flat_adam_step_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, uint16_t* __restrict__ shadow,  // null: no shadow
    const double* __restrict__ partial, int G, const int64_t* __restrict__ step_next,
    int64_t* __restrict__ step, const float* __restrict__ lr, float* __restrict__ norm_out,
    int64_t N, double beta1, double beta2, float eps, float max_norm, int clip) {
#pragma clang fp contract(off)
  __shared__ double sWave[kWaves];
  __shared__ double sTotal;
  const int tid = threadIdx.x;

  // The same order in every block: thread i takes partial[i], [i + 256], ...
  double acc = 0.0;
  for (int i = tid; i < G; i += kThreads) acc = acc + partial[i];
  const double S = blockSumF64(acc, sWave, &sTotal);
  const float norm = (float)sqrt(S);

  const int64_t t = *step_next;
  AdamScalars s;
  s.coef = 1.f;
  if (clip) {
    const float c = max_norm / (norm + 1e-6f);
    s.coef = c > 1.f ? 1.f : c;  // a NaN norm stays NaN, as torch.clamp keeps it
  }
  s.w1 = (float)(1.0 - beta1);
  s.beta2 = (float)beta2;
  s.w2 = (float)(1.0 - beta2);
  const float bc1 = (float)(1.0 - powInt(beta1, t));
  const float bc2 = (float)(1.0 - powInt(beta2, t));
  s.stepSize = *lr / bc1;
  s.bc2Sqrt = sqrtf(bc2);
  s.eps = eps;

  if (blockIdx.x == 0 && tid == 0) {
    *norm_out = norm;
    *step = t;
  }

  const int64_t nquad = (N + 3) / 4;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t q = (int64_t)blockIdx.x * kThreads + tid; q < nquad; q += stride) {
    const int64_t i = q * 4;
    if (i + 4 <= N) {
      const float4 gq = *reinterpret_cast<const float4*>(g + i);
      float4 pq = *reinterpret_cast<const float4*>(p + i);
      float4 mq = *reinterpret_cast<const float4*>(m + i);
      float4 vq = *reinterpret_cast<const float4*>(v + i);
      adamElement(s, gq.x, pq.x, mq.x, vq.x);
      adamElement(s, gq.y, pq.y, mq.y, vq.y);
      adamElement(s, gq.z, pq.z, mq.z, vq.z);
      adamElement(s, gq.w, pq.w, mq.w, vq.w);
      *reinterpret_cast<float4*>(p + i) = pq;
      *reinterpret_cast<float4*>(m + i) = mq;
      *reinterpret_cast<float4*>(v + i) = vq;
      if (shadow != nullptr) {
        uint2 packed;
        packed.x = bf16Bits(pq.x) | (bf16Bits(pq.y) << 16);
        packed.y = bf16Bits(pq.z) | (bf16Bits(pq.w) << 16);
        *reinterpret_cast<uint2*>(shadow + i) = packed;
      }
    } else {
      for (int64_t j = i; j < N; ++j) {
        float pj = p[j], mj = m[j], vj = v[j];
        adamElement(s, g[j], pj, mj, vj);
        p[j] = pj;
        m[j] = mj;
        v[j] = vj;
        if (shadow != nullptr) shadow[j] = (uint16_t)bf16Bits(pj);
      }
    }
  }
}

}  // namespace optim

// One fused Adam step over flat buffers; two launches on the current stream.
// `step` holds the number of steps taken so far and is advanced by one;
// `step_next` is the second word of the counter's ping-pong; `partial` is the
// per-block workspace of the norm; `norm_out` receives the unclipped norm.
void flat_adam_step(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v,
                    c10::optional<at::Tensor> shadow, at::Tensor step, at::Tensor step_next,
                    at::Tensor lr, at::Tensor partial, at::Tensor norm_out, double beta1,
                    double beta2, double eps, c10::optional<double> max_norm) {
  TORCH_CHECK(p.defined() && p.is_cuda() && p.scalar_type() == at::kFloat && p.dim() == 1 &&
                  p.is_contiguous(),
              "flat_adam_step: p must be a contiguous 1-D float32 CUDA tensor");
  const int64_t N = p.numel();
  TORCH_CHECK(N >= 1, "flat_adam_step: p must hold at least one element");
  auto check = [&](const at::Tensor& t, at::ScalarType dtype, int64_t minNumel, bool exact,
                   size_t align, const char* name) {
    TORCH_CHECK(t.defined() && t.is_cuda() && t.device() == p.device(), "flat_adam_step: ", name,
                " must be on the same CUDA device as p");
    TORCH_CHECK(t.scalar_type() == dtype, "flat_adam_step: ", name, " must be ", dtype, ", got ",
                t.scalar_type());
    TORCH_CHECK(t.is_contiguous(), "flat_adam_step: ", name, " must be contiguous");
    TORCH_CHECK(exact ? t.numel() == minNumel : t.numel() >= minNumel, "flat_adam_step: ", name,
                " must hold ", exact ? "" : "at least ", minNumel, " elements, got ", t.numel());
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % align == 0, "flat_adam_step: ", name,
                " must be ", align, "-byte aligned");
  };
  check(p, at::kFloat, N, true, 16, "p");
  check(g, at::kFloat, N, true, 16, "g");
  check(m, at::kFloat, N, true, 16, "m");
  check(v, at::kFloat, N, true, 16, "v");
  TORCH_CHECK(g.dim() == 1 && m.dim() == 1 && v.dim() == 1,
              "flat_adam_step: g, m and v must be 1-D like p");
  uint16_t* shadowPtr = nullptr;
  if (shadow.has_value() && shadow->defined()) {
    check(*shadow, at::kBFloat16, N, true, 8, "shadow");
    shadowPtr = reinterpret_cast<uint16_t*>(shadow->data_ptr());
  }
  check(step, at::kLong, 1, true, 8, "step");
  check(step_next, at::kLong, 1, true, 8, "step_next");
  TORCH_CHECK(step.data_ptr() != step_next.data_ptr(),
              "flat_adam_step: step and step_next must be two different words");
  check(lr, at::kFloat, 1, true, 4, "lr");
  check(partial, at::kDouble, optim::kMaxBlocks, false, 8, "partial");
  check(norm_out, at::kFloat, 1, true, 4, "norm_out");
  TORCH_CHECK(beta1 >= 0.0 && beta1 < 1.0, "flat_adam_step: beta1 must be in [0,1), got ", beta1);
  TORCH_CHECK(beta2 >= 0.0 && beta2 < 1.0, "flat_adam_step: beta2 must be in [0,1), got ", beta2);
  TORCH_CHECK(eps >= 0.0, "flat_adam_step: eps must be >= 0, got ", eps);
  const bool clip = max_norm.has_value();
  TORCH_CHECK(!clip || *max_norm > 0.0, "flat_adam_step: max_norm must be > 0 or None, got ",
              clip ? *max_norm : 0.0);

  const int G = optim::gridBlocks(N);
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(optim::flat_sumsq_kernel, dim3((unsigned)G), dim3(optim::kThreads), 0,
                     stream, g.data_ptr<float>(), partial.data_ptr<double>(),
                     step.data_ptr<int64_t>(), step_next.data_ptr<int64_t>(), N);
  hipLaunchKernelGGL(optim::flat_adam_step_kernel, dim3((unsigned)G), dim3(optim::kThreads), 0,
                     stream, p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
                     v.data_ptr<float>(), shadowPtr, partial.data_ptr<double>(), G,
                     step_next.data_ptr<int64_t>(), step.data_ptr<int64_t>(),
                     lr.data_ptr<float>(), norm_out.data_ptr<float>(), N, beta1, beta2,
                     (float)eps, clip ? (float)*max_norm : 0.f, clip ? 1 : 0);
}
