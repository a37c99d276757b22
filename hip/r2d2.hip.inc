// Fused R2D2 loss for gfx950 — included by kernels.hip.
//
// n-step double-Q targets under the invertible value rescaling h, the masked
// sequence loss, the mixed max/mean sequence priority AND the analytic
// gradient w.r.t. the online Q-values (Kapturowski et al. 2019), in ONE
// launch. The eager path (moolib_amd/ops/r2d2.py) is an n-step Python loop of
// small [T,B] ops plus an autograd graph; [T,B,A] is tiny (80x64x18), so
// like vtrace_scan_kernel this is launch-latency elimination, not FLOPs.
//
//   - grid: one workgroup per sequence b, 256 threads (4 waves);
//   - phase 1: waves stride over t. Each does a wave-wide (value, index)
//     argmax of q[t,b,:] (lowest index wins ties), zero-fills the grad_q row
//     except the taken action's element, and lane 0 stages
//     boot_t = h^-1(q_target[t,b,a*]) and q[t,b,a_t] in LDS; reward,
//     discount and mask of the column are staged in LDS too;
//   - phase 2 (after a barrier): thread t forms the n-step return G_t from
//     LDS and writes td[t,b] and the one non-zero gradient element;
//   - phase 3: block reduction (shuffles + LDS, NO atomics) -> loss_seq[b],
//     priority[b].
// Every grad_q element is written exactly once (no memset, no ordering
// between two writers), every input is read once, and the result is
// bit-reproducible from run to run.
//
// Numerics: IEEE sqrtf and division, no fast intrinsics, and fp contraction
// is switched off so that td and grad_q round like the fp32 eager path, which
// performs the same operations in the same order. The per-sequence sums
// accumulate in fp64.

namespace r2d2 {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
// Phase 2 gives each step its own thread and the column lives in LDS
// (6 arrays x 256 x 4 B = 6 KiB of LDS): sequences of up to 256 network steps.
constexpr int kMaxT = kThreads;

DEV_INLINE float signOf(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

DEV_INLINE double waveReduceSumF64(double v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
  return v;  // lane 0 holds the sum
}

// h(x) = sign(x)(sqrt(|x|+1) - 1) + eps x
DEV_INLINE float rescaleValue(float x, float eps) {
#pragma clang fp contract(off)
  float root = sqrtf(fabsf(x) + 1.f) - 1.f;
  float lin = eps * x;
  return signOf(x) * root + lin;
}

// h^-1(x) = sign(x)(s^2 - 1), s = 2a / (sqrt(1 + 4 eps a) + 1), a = |x| + 1 + eps:
// the cancellation-free form of ((sqrt(1 + 4 eps a) - 1) / (2 eps))^2 - 1.
DEV_INLINE float inverseRescaleValue(float x, float eps, float fourEps) {
#pragma clang fp contract(off)
  float a = fabsf(x) + 1.f + eps;
  float t = fourEps * a;
  float s = (2.f * a) / (sqrtf(1.f + t) + 1.f);
  float s2 = s * s;
  return signOf(x) * (s2 - 1.f);
}

__global__ __launch_bounds__(kThreads) void r2d2_loss_kernel(
    const float* __restrict__ q,          // [T,B,A] online
    const float* __restrict__ q_target,   // [T,B,A] target
    const int64_t* __restrict__ actions,  // [T,B]
    const float* __restrict__ rewards,    // [T,B]
    const float* __restrict__ discounts,  // [T,B]
    const float* __restrict__ mask,       // [T,B]
    const float* __restrict__ is_weights, // [B]
    float* __restrict__ td,               // [T,B]
    float* __restrict__ loss_seq,         // [B]
    float* __restrict__ priority,         // [B]
    float* __restrict__ grad_q,           // [T,B,A]
    int T, int B, int A, int n, float eps, int rescale, float eta, float oneMinusEta,
    float grad_scale) {
#pragma clang fp contract(off)
  __shared__ float sBoot[kMaxT];
  __shared__ float sQa[kMaxT];
  __shared__ float sReward[kMaxT];
  __shared__ float sDiscount[kMaxT];
  __shared__ float sMask[kMaxT];
  __shared__ int sAction[kMaxT];
  __shared__ double sSum[3][kWaves];
  __shared__ float sMax[kWaves];

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid % kWave;
  const int wave = tid / kWave;
  const float fourEps = 4.f * eps;

  if (tid < T) {
    const int64_t i = (int64_t)tid * B + b;
    sReward[tid] = rewards[i];
    sDiscount[tid] = discounts[i];
    sMask[tid] = mask[i];
  }

  // ---- phase 1: per-step argmax / bootstrap / taken-action value
  for (int t = wave; t < T; t += kWaves) {
    const int64_t row = ((int64_t)t * B + b) * A;
    const float* qrow = q + row;
    float* grow = grad_q + row;
    int64_t a64 = actions[(int64_t)t * B + b];
    // Defensive clamp (as in impala_loss_kernel): a corrupted batch must not
    // read or write out of bounds.
    const int a = (a64 < 0 || a64 >= A) ? 0 : (int)a64;

    float bestV = -INFINITY;
    int bestI = INT_MAX;  // "no element yet"
    float qa = 0.f;
    for (int j = lane; j < A; j += kWave) {
      float v = qrow[j];
      if (bestI == INT_MAX || v > bestV) {
        bestV = v;
        bestI = j;
      }
      if (j == a) {
        qa = v;
      } else {
        grow[j] = 0.f;
      }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      float otherV = __shfl_down(bestV, off);
      int otherI = __shfl_down(bestI, off);
      if (otherV > bestV || (otherV == bestV && otherI < bestI)) {
        bestV = otherV;
        bestI = otherI;
      }
    }
    bestI = __shfl(bestI, 0);
    if (bestI < 0 || bestI >= A) bestI = 0;
    qa = __shfl(qa, a % kWave);
    if (lane == 0) {
      float boot = q_target[row + bestI];
      sBoot[t] = rescale ? inverseRescaleValue(boot, eps, fourEps) : boot;
      sQa[t] = qa;
      sAction[t] = a;
    }
  }
  __syncthreads();

  // ---- phase 2: n-step return and TD error of step t = tid
  float delta = 0.f;
  float valid = 0.f;
  if (tid < T - 1) {
    const int t = tid;
    const int k = min(n, T - 1 - t);
    float G = 0.f;
    float disc = 1.f;
    for (int i = 0; i < k; ++i) {
      G = G + disc * sReward[t + i];
      disc = disc * sDiscount[t + i];
    }
    G = G + disc * sBoot[t + k];
    if (rescale) G = rescaleValue(G, eps);
    valid = sMask[t];
    delta = valid * (G - sQa[t]);
  }
  if (tid < T) {
    const int64_t i = (int64_t)tid * B + b;
    td[i] = delta;
    grad_q[i * A + sAction[tid]] = -(grad_scale * is_weights[b]) * delta;
  }

  // ---- phase 3: sequence loss and priority. The sums run in fp64 in a fixed
  // order (their rounding error is far below one fp32 ulp of the result) and
  // are rounded to fp32 once.
  const float absDelta = fabsf(delta);
  double sumSq = waveReduceSumF64((double)(delta * delta));
  double sumAbs = waveReduceSumF64((double)absDelta);
  double sumValid = waveReduceSumF64((double)valid);
  float maxAbs = waveReduceMax(absDelta);
  if (lane == 0) {
    sSum[0][wave] = sumSq;
    sSum[1][wave] = sumAbs;
    sSum[2][wave] = sumValid;
    sMax[wave] = maxAbs;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kWaves; ++w) {
      sumSq = sumSq + sSum[0][w];
      sumAbs = sumAbs + sSum[1][w];
      sumValid = sumValid + sSum[2][w];
      maxAbs = fmaxf(maxAbs, sMax[w]);
    }
    loss_seq[b] = 0.5f * (float)sumSq;
    float meanAbs = (float)sumAbs / fmaxf(1.f, (float)sumValid);
    priority[b] = eta * maxAbs + oneMinusEta * meanAbs;
  }
}

// Initial priority of an actor's sequence from its own Q-values: the loss
// kernel without the argmax phase and without a gradient. Inputs are in the
// actor's layout, reward[t] and done[t] arrive WITH step t, so the reward and
// discount that follow action t are read from row t+1 here; the last row has
// no successor and only bootstraps.
//   - grid: one workgroup per environment k, 256 threads, thread t owns step t;
//   - thread t stages boot_t = h^-1(q_max[t,k]), q_taken[t,k], r_t, g_t in LDS;
//   - after a barrier it forms G_t and writes td[t,k] (zero for t = T-1 and
//     for burn-in steps);
//   - the block reduction of r2d2_loss_kernel writes priority[k].
// Every output element is written exactly once, no atomics, no memset.
__global__ __launch_bounds__(kThreads) void actor_priority_kernel(
    const float* __restrict__ q_taken,  // [T,K]
    const float* __restrict__ q_max,    // [T,K]
    const float* __restrict__ reward,   // [T,K]
    const uint8_t* __restrict__ done,   // [T,K], bool or uint8
    float* __restrict__ td,             // [T,K]
    float* __restrict__ priority,       // [K]
    int T, int K, int n, int burn_in, float discount, float eps, int rescale, float eta,
    float oneMinusEta) {
#pragma clang fp contract(off)
  __shared__ float sBoot[kMaxT];
  __shared__ float sQa[kMaxT];
  __shared__ float sReward[kMaxT];
  __shared__ float sDiscount[kMaxT];
  __shared__ double sSum[2][kWaves];
  __shared__ float sMax[kWaves];

  const int k = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid % kWave;
  const int wave = tid / kWave;

  if (tid < T) {
    const int64_t i = (int64_t)tid * K + k;
    const float boot = q_max[i];
    sBoot[tid] = rescale ? inverseRescaleValue(boot, eps, 4.f * eps) : boot;
    sQa[tid] = q_taken[i];
    const bool more = tid < T - 1;  // row t+1 exists
    sReward[tid] = more ? reward[i + K] : 0.f;
    sDiscount[tid] = (more && done[i + K] == 0) ? discount : 0.f;
  }
  __syncthreads();

  float delta = 0.f;
  float valid = 0.f;
  if (tid < T - 1) {
    const int t = tid;
    const int steps = min(n, T - 1 - t);
    float G = 0.f;
    float disc = 1.f;
    for (int i = 0; i < steps; ++i) {
      G = G + disc * sReward[t + i];
      disc = disc * sDiscount[t + i];
    }
    G = G + disc * sBoot[t + steps];
    if (rescale) G = rescaleValue(G, eps);
    valid = t >= burn_in ? 1.f : 0.f;
    delta = valid * (G - sQa[t]);
  }
  if (tid < T) td[(int64_t)tid * K + k] = delta;

  const float absDelta = fabsf(delta);
  double sumAbs = waveReduceSumF64((double)absDelta);
  double sumValid = waveReduceSumF64((double)valid);
  float maxAbs = waveReduceMax(absDelta);
  if (lane == 0) {
    sSum[0][wave] = sumAbs;
    sSum[1][wave] = sumValid;
    sMax[wave] = maxAbs;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kWaves; ++w) {
      sumAbs = sumAbs + sSum[0][w];
      sumValid = sumValid + sSum[1][w];
      maxAbs = fmaxf(maxAbs, sMax[w]);
    }
    float meanAbs = (float)sumAbs / fmaxf(1.f, (float)sumValid);
    priority[k] = eta * maxAbs + oneMinusEta * meanAbs;
  }
}

}  // namespace r2d2

// priority [K], td [T,K] of an actor's sequences, in the actor's layout
// (reward[t], done[t] arrive with step t). `priority_out` / `td_out`, if given,
// are the buffers the results are written into (every element).
std::vector<at::Tensor> r2d2_actor_priority(at::Tensor q_taken, at::Tensor q_max,
                                            at::Tensor reward, at::Tensor done, int64_t n,
                                            double discount, double eps, bool rescale,
                                            double eta, int64_t burn_in,
                                            c10::optional<at::Tensor> priority_out,
                                            c10::optional<at::Tensor> td_out) {
  TORCH_CHECK(q_taken.defined() && q_taken.is_cuda() && q_taken.scalar_type() == at::kFloat &&
                  q_taken.dim() == 2 && q_taken.is_contiguous(),
              "r2d2_actor_priority: q_taken must be a contiguous float32 CUDA tensor [T,K]");
  const int64_t T = q_taken.size(0), K = q_taken.size(1);
  TORCH_CHECK(T >= 1 && K >= 1, "r2d2_actor_priority: q_taken must be non-empty, got ",
              q_taken.sizes());
  TORCH_CHECK(T <= r2d2::kMaxT, "r2d2_actor_priority: T = ", T,
              " exceeds the kernel's limit of ", r2d2::kMaxT, " steps per sequence");
  TORCH_CHECK(K <= INT_MAX, "r2d2_actor_priority: K must fit in int32");
  TORCH_CHECK(n >= 1, "r2d2_actor_priority: n_step must be >= 1, got ", n);
  TORCH_CHECK(eps >= 0.0, "r2d2_actor_priority: eps must be >= 0, got ", eps);
  TORCH_CHECK(eta >= 0.0 && eta <= 1.0, "r2d2_actor_priority: eta must be in [0,1], got ", eta);
  TORCH_CHECK(burn_in >= 0, "r2d2_actor_priority: burn_in must be >= 0, got ", burn_in);
  auto check = [&](const at::Tensor& t, bool flag, at::IntArrayRef shape, const char* name) {
    TORCH_CHECK(t.defined() && t.is_cuda() && t.device() == q_taken.device(),
                "r2d2_actor_priority: ", name, " must be on the same CUDA device as q_taken");
    if (flag) {
      TORCH_CHECK(t.scalar_type() == at::kBool || t.scalar_type() == at::kByte,
                  "r2d2_actor_priority: ", name, " must be bool or uint8, got ", t.scalar_type());
    } else {
      TORCH_CHECK(t.scalar_type() == at::kFloat, "r2d2_actor_priority: ", name,
                  " must be Float, got ", t.scalar_type());
    }
    TORCH_CHECK(t.sizes() == shape, "r2d2_actor_priority: ", name, " must have shape ", shape,
                ", got ", t.sizes());
    TORCH_CHECK(t.is_contiguous(), "r2d2_actor_priority: ", name, " must be contiguous");
  };
  check(q_max, false, {T, K}, "q_max");
  check(reward, false, {T, K}, "reward");
  check(done, true, {T, K}, "done");
  at::Tensor priority, td;
  if (priority_out.has_value() && priority_out->defined()) {
    check(*priority_out, false, {K}, "priority_out");
    priority = *priority_out;
  } else {
    priority = at::empty({K}, q_taken.options());
  }
  if (td_out.has_value() && td_out->defined()) {
    check(*td_out, false, {T, K}, "td_out");
    td = *td_out;
  } else {
    td = at::empty({T, K}, q_taken.options());
  }
  // windows end at T-1 and no step past it is valid anyway
  const int nSteps = (int)std::min<int64_t>(n, r2d2::kMaxT);
  const int burnIn = (int)std::min<int64_t>(burn_in, r2d2::kMaxT);
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(r2d2::actor_priority_kernel, dim3((unsigned)K), dim3(r2d2::kThreads), 0,
                     stream, q_taken.data_ptr<float>(), q_max.data_ptr<float>(),
                     reward.data_ptr<float>(), static_cast<const uint8_t*>(done.data_ptr()),
                     td.data_ptr<float>(), priority.data_ptr<float>(), (int)T, (int)K, nSteps,
                     burnIn, (float)discount, (float)eps, rescale ? 1 : 0, (float)eta,
                     (float)(1.0 - eta));
  return {priority, td};
}

// td [T,B], loss_seq [B], priority [B], grad_q [T,B,A]. `grad_out`, if given,
// is the [T,B,A] buffer the gradient is written into (every element).
std::vector<at::Tensor> r2d2_loss(at::Tensor q, at::Tensor q_target, at::Tensor actions,
                                  at::Tensor rewards, at::Tensor discounts, at::Tensor mask,
                                  at::Tensor is_weights, int64_t n, double eps, bool rescale,
                                  double eta, double grad_scale,
                                  c10::optional<at::Tensor> grad_out) {
  TORCH_CHECK(q.defined() && q.is_cuda() && q.scalar_type() == at::kFloat && q.dim() == 3 &&
                  q.is_contiguous(),
              "r2d2_loss: q must be a contiguous float32 CUDA tensor [T,B,A]");
  const int64_t T = q.size(0), B = q.size(1), A = q.size(2);
  TORCH_CHECK(T >= 1 && B >= 1 && A >= 1, "r2d2_loss: q must be non-empty, got ", q.sizes());
  TORCH_CHECK(T <= r2d2::kMaxT, "r2d2_loss: T = ", T, " exceeds the kernel's limit of ",
              r2d2::kMaxT, " steps per sequence");
  TORCH_CHECK(B <= INT_MAX && A <= INT_MAX, "r2d2_loss: B and A must fit in int32");
  TORCH_CHECK(n >= 1, "r2d2_loss: n_step must be >= 1, got ", n);
  TORCH_CHECK(eps >= 0.0, "r2d2_loss: eps must be >= 0, got ", eps);
  TORCH_CHECK(eta >= 0.0 && eta <= 1.0, "r2d2_loss: eta must be in [0,1], got ", eta);
  // the kernel indexes every operand from T, B and A alone
  auto check = [&](const at::Tensor& t, at::ScalarType dtype, at::IntArrayRef shape,
                   const char* name) {
    TORCH_CHECK(t.defined() && t.is_cuda() && t.device() == q.device(), "r2d2_loss: ", name,
                " must be on the same CUDA device as q");
    TORCH_CHECK(t.scalar_type() == dtype, "r2d2_loss: ", name, " must be ", dtype, ", got ",
                t.scalar_type());
    TORCH_CHECK(t.sizes() == shape, "r2d2_loss: ", name, " must have shape ", shape, ", got ",
                t.sizes());
    TORCH_CHECK(t.is_contiguous(), "r2d2_loss: ", name, " must be contiguous");
  };
  check(q_target, at::kFloat, {T, B, A}, "q_target");
  check(actions, at::kLong, {T, B}, "actions");
  check(rewards, at::kFloat, {T, B}, "rewards");
  check(discounts, at::kFloat, {T, B}, "discounts");
  check(mask, at::kFloat, {T, B}, "mask");
  check(is_weights, at::kFloat, {B}, "is_weights");
  at::Tensor grad_q;
  if (grad_out.has_value() && grad_out->defined()) {
    check(*grad_out, at::kFloat, {T, B, A}, "grad_out");
    grad_q = *grad_out;
  } else {
    grad_q = at::empty_like(q);
  }
  auto td = at::empty({T, B}, q.options());
  auto loss_seq = at::empty({B}, q.options());
  auto priority = at::empty({B}, q.options());
  const int nSteps = (int)std::min<int64_t>(n, r2d2::kMaxT);  // windows end at T-1 anyway
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(r2d2::r2d2_loss_kernel, dim3((unsigned)B), dim3(r2d2::kThreads), 0, stream,
                     q.data_ptr<float>(), q_target.data_ptr<float>(),
                     actions.data_ptr<int64_t>(), rewards.data_ptr<float>(),
                     discounts.data_ptr<float>(), mask.data_ptr<float>(),
                     is_weights.data_ptr<float>(), td.data_ptr<float>(),
                     loss_seq.data_ptr<float>(), priority.data_ptr<float>(),
                     grad_q.data_ptr<float>(), (int)T, (int)B, (int)A, nSteps, (float)eps,
                     rescale ? 1 : 0, (float)eta, (float)(1.0 - eta), (float)grad_scale);
  return {td, loss_seq, priority, grad_q};
}
