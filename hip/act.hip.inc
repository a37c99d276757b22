// Fused actor head for gfx950 — included by kernels.hip.
//
// Two small latency-bound kernels that end an actor step in ONE launch of our
// own each, with no torch generator behind them:
//
//   act_categorical  action ~ softmax(logits), by inversion of the ordered
//                    fp32 CDF of exp(l - max);
//   act_eps_greedy   dueling Q = V + A - mean A, its greedy action, an
//                    epsilon-greedy draw per row, Q of the action taken and
//                    of the greedy one.
//
// Random numbers are counter-based: the whole sampler state is two int64 on
// the device, [seed, step]. A launch reads `step`, draws Philox4x32-10 with
//   key = (seed lo, seed hi), counter = (row, 0, step lo, step hi),
// takes u0 = (x0 >> 8) 2^-24 and u1 = (x1 >> 8) 2^-24 (x2, x3 unused), and
// stores step + 1: a captured launch draws fresh numbers on every replay, and
// any draw can be recomputed on the CPU from (seed, step, row). With explicit
// uniforms u [N, 2] the state is neither read nor advanced.
//
// Each kernel is ONE workgroup: threads stride over the N rows, one row per
// thread per pass. All threads read `step` before the first barrier; after
// the last one thread 0 stores step + 1 with an ordinary vector store. No
// atomics, no fast intrinsics, fp contraction off, IEEE division. The row
// stays in memory and is re-read per pass (a dynamically indexed register
// array would go to scratch); expf of the same input gives the same value, so
// the scan is self-consistent. moolib_amd/ops/act.py holds the definition and
// a plain-torch path that performs the same operations in the same order.

namespace act {

constexpr int kThreads = 1024;
// Most actions a row may hold. Larger A is rejected on the host.
constexpr int kMaxActions = 64;

struct Uniforms {
  float u0, u1;
};

DEV_INLINE Uniforms philoxUniforms(uint64_t seed, uint64_t step, uint32_t row) {
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;
  constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t c0 = row, c1 = 0u, c2 = (uint32_t)step, c3 = (uint32_t)(step >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kM0 * c0;
    const uint64_t p1 = (uint64_t)kM1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += kW0;
    k1 += kW1;
  }
  Uniforms u;
  u.u0 = (float)(c0 >> 8) * 0x1p-24f;  // 24 bits: exact
  u.u1 = (float)(c1 >> 8) * 0x1p-24f;
  return u;
}

// The uniforms of row n: explicit, or drawn from (seed, step, n).
DEV_INLINE Uniforms rowUniforms(const float* __restrict__ u, uint64_t seed, uint64_t step,
                                int64_t n) {
  if (u != nullptr) {
    Uniforms r;
    r.u0 = u[2 * n];
    r.u1 = u[2 * n + 1];
    return r;
  }
  return philoxUniforms(seed, step, (uint32_t)n);
}

// state is read before the first barrier and written after the last.
__global__ __launch_bounds__(kThreads) void act_categorical_kernel(
    const float* __restrict__ logits,  // [N, A]
    const float* __restrict__ u,       // [N, 2] or null: draw from state
    int64_t* state,                    // [2] = seed, step; or null with u
    int64_t* __restrict__ action,      // [N]
    int64_t N, int A) {
#pragma clang fp contract(off)
  uint64_t seed = 0, step = 0;
  if (state != nullptr) {
    seed = (uint64_t)state[0];
    step = (uint64_t)state[1];
  }
  __syncthreads();
  for (int64_t n = threadIdx.x; n < N; n += kThreads) {
    const float* __restrict__ row = logits + n * A;
    const Uniforms r = rowUniforms(u, seed, step, n);
    float m = row[0];
    for (int a = 1; a < A; ++a) m = fmaxf(m, row[a]);
    float total = 0.f;
    int last = 0;  // last action of non-zero probability
    for (int a = 0; a < A; ++a) {
      const float e = expf(row[a] - m);
      total = total + e;
      if (e > 0.f) last = a;
    }
    const float target = r.u0 * total;
    float c = 0.f;
    int pick = last;  // rounding at the top: no running sum exceeds target
    for (int a = 0; a < A; ++a) {
      c = c + expf(row[a] - m);
      if (c > target) {
        pick = a;
        break;
      }
    }
    action[n] = pick;
  }
  __syncthreads();
  if (state != nullptr && threadIdx.x == 0) state[1] = (int64_t)(step + 1);
}

__global__ __launch_bounds__(kThreads) void act_eps_greedy_kernel(
    const float* __restrict__ value,      // [N]
    const float* __restrict__ advantage,  // [N, A]
    const float* __restrict__ epsilon,    // [N]
    const float* __restrict__ u,          // [N, 2] or null: draw from state
    int64_t* state,                       // [2] = seed, step; or null with u
    int64_t* __restrict__ action,         // [N]
    float* __restrict__ q_taken,          // [N]
    float* __restrict__ q_max,            // [N]
    int64_t N, int A) {
#pragma clang fp contract(off)
  uint64_t seed = 0, step = 0;
  if (state != nullptr) {
    seed = (uint64_t)state[0];
    step = (uint64_t)state[1];
  }
  __syncthreads();
  for (int64_t n = threadIdx.x; n < N; n += kThreads) {
    const float* __restrict__ row = advantage + n * A;
    const Uniforms r = rowUniforms(u, seed, step, n);
    float s = 0.f;
    for (int a = 0; a < A; ++a) s = s + row[a];
    const float mean = s / (float)A;
    const float v = value[n];
    int greedy = 0;
    float best = (v + row[0]) - mean;
    for (int a = 1; a < A; ++a) {
      const float q = (v + row[a]) - mean;
      if (q > best) {  // strict: the lowest index of the maximum wins
        best = q;
        greedy = a;
      }
    }
    const bool explore = r.u0 < epsilon[n];
    const int random_action = min(A - 1, (int)floorf(r.u1 * (float)A));
    const int a = explore ? random_action : greedy;
    action[n] = a;
    q_taken[n] = (v + row[a]) - mean;
    q_max[n] = best;
  }
  __syncthreads();
  if (state != nullptr && threadIdx.x == 0) state[1] = (int64_t)(step + 1);
}

// Exactly one of `state` (int64 [2]) and `u` (float32 [N, 2]); returns the
// raw pointers through `statePtr` / `uPtr`.
inline void checkSource(const c10::optional<at::Tensor>& state, const c10::optional<at::Tensor>& u,
                        const at::Tensor& like, int64_t N, const char* fn, int64_t** statePtr,
                        const float** uPtr) {
  const bool hasState = state.has_value() && state->defined();
  const bool hasU = u.has_value() && u->defined();
  TORCH_CHECK(hasState != hasU, fn, ": exactly one of state and u must be given");
  *statePtr = nullptr;
  *uPtr = nullptr;
  if (hasState) {
    const at::Tensor& s = *state;
    TORCH_CHECK(s.is_cuda() && s.device() == like.device() && s.scalar_type() == at::kLong &&
                    s.dim() == 1 && s.numel() == 2 && s.is_contiguous(),
                fn, ": state must be a contiguous int64 [2] tensor on the input's device");
    *statePtr = s.data_ptr<int64_t>();
  } else {
    const at::Tensor& t = *u;
    TORCH_CHECK(t.is_cuda() && t.device() == like.device() && t.scalar_type() == at::kFloat &&
                    t.dim() == 2 && t.size(0) == N && t.size(1) == 2 && t.is_contiguous(),
                fn, ": u must be a contiguous float32 [N, 2] tensor on the input's device");
    *uPtr = t.data_ptr<float>();
  }
}

// The [N] output buffer `out` if given (checked), else a fresh one.
inline at::Tensor outVec(const c10::optional<at::Tensor>& out, const at::Tensor& like, int64_t N,
                         at::ScalarType dtype, const char* fn, const char* name) {
  if (!(out.has_value() && out->defined())) return at::empty({N}, like.options().dtype(dtype));
  const at::Tensor& o = *out;
  TORCH_CHECK(o.is_cuda() && o.device() == like.device() && o.scalar_type() == dtype &&
                  o.dim() == 1 && o.numel() == N && o.is_contiguous(),
              fn, ": ", name, " must be a contiguous ", dtype, " [N] tensor on the input's device");
  return o;
}

inline void checkRows(const at::Tensor& x, const char* fn, const char* name) {
  TORCH_CHECK(x.defined() && x.is_cuda() && x.scalar_type() == at::kFloat && x.dim() == 2 &&
                  x.is_contiguous(),
              fn, ": ", name, " must be a contiguous float32 [N, A] CUDA tensor");
  TORCH_CHECK(x.size(0) >= 1 && x.size(0) <= (int64_t)INT_MAX, fn, ": N must be in [1, 2^31), got ",
              x.size(0));
  TORCH_CHECK(x.size(1) >= 1 && x.size(1) <= kMaxActions, fn, ": A must be in [1, ", kMaxActions,
              "], got ", x.size(1));
}

}  // namespace act

// action[n] ~ softmax(logits[n]) by inversion of the ordered fp32 CDF, driven
// by state = [seed, step] (advanced by one) or by explicit uniforms u [N, 2].
// `action_out`, if given, is the int64 [N] buffer written into.
at::Tensor act_categorical(at::Tensor logits, c10::optional<at::Tensor> state,
                           c10::optional<at::Tensor> u, c10::optional<at::Tensor> action_out) {
  act::checkRows(logits, "act_categorical", "logits");
  const int64_t N = logits.size(0);
  const int A = (int)logits.size(1);
  int64_t* statePtr;
  const float* uPtr;
  act::checkSource(state, u, logits, N, "act_categorical", &statePtr, &uPtr);
  at::Tensor action = act::outVec(action_out, logits, N, at::kLong, "act_categorical", "action_out");
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(act::act_categorical_kernel, dim3(1), dim3(act::kThreads), 0, stream,
                     logits.data_ptr<float>(), uPtr, statePtr, action.data_ptr<int64_t>(), N, A);
  return action;
}

// Epsilon-greedy action on the dueling Q-values of (value [N], advantage
// [N, A]) with one epsilon per row: (action int64 [N], q_taken [N], q_max [N]),
// written into the `*_out` buffers where given.
std::vector<at::Tensor> act_eps_greedy(at::Tensor value, at::Tensor advantage, at::Tensor epsilon,
                                       c10::optional<at::Tensor> state,
                                       c10::optional<at::Tensor> u,
                                       c10::optional<at::Tensor> action_out,
                                       c10::optional<at::Tensor> q_taken_out,
                                       c10::optional<at::Tensor> q_max_out) {
  act::checkRows(advantage, "act_eps_greedy", "advantage");
  const int64_t N = advantage.size(0);
  const int A = (int)advantage.size(1);
  auto checkVec = [&](const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.defined() && t.is_cuda() && t.device() == advantage.device() &&
                    t.scalar_type() == at::kFloat && t.dim() == 1 && t.numel() == N &&
                    t.is_contiguous(),
                "act_eps_greedy: ", name,
                " must be a contiguous float32 [N] tensor on advantage's device");
  };
  checkVec(value, "value");
  checkVec(epsilon, "epsilon");
  int64_t* statePtr;
  const float* uPtr;
  act::checkSource(state, u, advantage, N, "act_eps_greedy", &statePtr, &uPtr);
  const char* fn = "act_eps_greedy";
  at::Tensor action = act::outVec(action_out, advantage, N, at::kLong, fn, "action_out");
  at::Tensor q_taken = act::outVec(q_taken_out, advantage, N, at::kFloat, fn, "q_taken_out");
  at::Tensor q_max = act::outVec(q_max_out, advantage, N, at::kFloat, fn, "q_max_out");
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(act::act_eps_greedy_kernel, dim3(1), dim3(act::kThreads), 0, stream,
                     value.data_ptr<float>(), advantage.data_ptr<float>(),
                     epsilon.data_ptr<float>(), uPtr, statePtr, action.data_ptr<int64_t>(),
                     q_taken.data_ptr<float>(), q_max.data_ptr<float>(), N, A);
  return {action, q_taken, q_max};
}
