// One trunk section after its section conv, for the actor (no grad), as ONE
// launch: 3x3/s2/p1 max-pool, then both residual blocks, with the pooled
// image resident in LDS (gfx950, 160 KB per workgroup).
//
// The two-launch-per-block route (conv3x3.hip.inc) sends every activation
// through HBM three times per conv and gathers nine taps per pixel from
// global memory on a grid too small to hide them; a pooled image is only
// 8..62 KB. Here one workgroup owns one image:
//
//   A, B: two zero-haloed LDS images [(OH+2)][(OW+2)][K] bf16
//   pool(u)                                  -> A   (raw x, the residual)
//   res0.conv0( relu(A + pending) on load )  -> B   stored as relu(. + b0)
//   res0.conv1( B )  + b1 + pending + A      -> A   in place
//   res1.conv0( relu(A) on load )            -> B   stored as relu(. + b0')
//   res1.conv1( B )  + b1' + A               -> A   in place
//   A (optionally relu'ed)                   -> out, 16-byte stores
//
// conv1 may overwrite A in place because each output reads only its own
// residual element and conv1's taps come from B. conv0's output has a
// single consumer, conv1's producer relu(u + b0), so it is stored with that
// producer already applied (after the bf16 rounding of u): conv1's nine tap
// reads are then plain LDS loads. conv0 cannot do the same, A must stay raw
// for the residual.
//
// Arithmetic is that of conv3x3_nhwc_kernel<K, true, 1>, bit for bit: same
// MFMA, same A/B fragment maps, kk ascending into accumulators kk&1 summed
// as acc[0]+acc[1], same producer and epilogue expressions and rounding
// points. Only where operands come from differs. No index plane is written.

namespace actor_section {

using conv3x3::bf16;
using conv3x3::bf16x8;
using conv3x3::floatx4;
using conv3x3::zero8;

// LDS per workgroup on gfx950; the host also asks the device.
constexpr int64_t kLdsMax = 160 * 1024;

struct Args {
  const bf16* u;        // [N, H, W, K] section conv output, short of `pending`
  const bf16* pending;  // [K] bias the section conv left out, or null
  const bf16* w[4];     // "fwd" packs of res0.conv0, res0.conv1, res1.conv0, res1.conv1
  const bf16* b[4];     // their biases, [K] each
  bf16* out;            // [N, OH, OW, K]
  int H, W, OH, OW;
  int reluOut;
};

// One conv over the resident image. FIRST (a block's conv0): src is raw, the
// producer relu(x + biasIn) runs on load and padding is zero AFTER it, so
// taps are bounds-checked; the output is rounded to bf16 bias-free and
// stored as conv1's producer relu(. + e1) of it. Otherwise (conv1): src
// already holds produced values inside a zero halo; the epilogue is
// v += e1 + e2 + residual with the residual read from, and the result
// written to, dst in place.
template <int K, bool FIRST>
C3_DEV void conv_pass(const bf16* src, bf16* dst, const bf16* __restrict__ wPacked,
                      const bf16* __restrict__ biasIn, const bf16* __restrict__ e1,
                      const bf16* __restrict__ e2, int OH, int OW) {
  constexpr int KK = (9 * K + 31) / 32;
  constexpr int NCT = K / 16;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int nWaves = blockDim.x >> 6;
  const int lo = lane & 15, hi = lane >> 4;
  const int WS = OW + 2;
  const int P = OH * OW;

  // The whole pack stays in registers for the pass: 5 fragments at K=16,
  // 18 at K=32.
  bf16x8 b[NCT][KK];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int kk = 0; kk < KK; ++kk)
      b[ct][kk] = *reinterpret_cast<const bf16x8*>(wPacked + ((ct * KK + kk) * 64 + lane) * 8);

  // A lane's 8 channels are the same in every chunk: 32 % K == 0.
  const int c0 = (hi * 8) % K;
  float bin[8];
  if (FIRST && biasIn != nullptr) {
#pragma unroll
    for (int e = 0; e < 8; ++e) bin[e] = (float)biasIn[c0 + e];
  }
  float f1[NCT], f2[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    f1[ct] = (float)e1[ct * 16 + lo];
    f2[ct] = (!FIRST && e2 != nullptr) ? (float)e2[ct * 16 + lo] : 0.f;
  }

  const int nTiles = (P + 15) / 16;
  for (int tile = wave; tile < nTiles; tile += nWaves) {
    const int p = tile * 16 + lo;  // this lane's A row
    const bool aok = p < P;
    const int pr = aok ? p / OW : 0;
    const int pc = aok ? p - pr * OW : 0;
    floatx4 acc[2][NCT];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch)
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) acc[ch][ct] = (floatx4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      const int tap = (kk * 32 + hi * 8) / K;
      bf16x8 a = zero8();
      if (aok && tap < 9) {
        const int dh = tap / 3, dw = tap % 3;
        // the -1 of the padding is the halo: image pixel (r, c) sits at (r+1, c+1)
        const bf16* sp = src + ((pr + dh) * WS + (pc + dw)) * K + c0;
        if (FIRST) {
          const int ih = pr + dh - 1, iw = pc + dw - 1;
          if (ih >= 0 && ih < OH && iw >= 0 && iw < OW) {
            a = *reinterpret_cast<const bf16x8*>(sp);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              float v = (float)a[e];
              if (biasIn != nullptr) v += bin[e];
              a[e] = (bf16)(v > 0.f ? v : 0.f);
            }
          }
        } else {
          a = *reinterpret_cast<const bf16x8*>(sp);
        }
      }
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
        acc[kk & 1][ct] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[ct][kk], acc[kk & 1][ct], 0, 0, 0);
    }

    // rows hi*4+reg, col ct*16+lo
    const int q = tile * 16 + hi * 4;
    int er = q / OW;
    int ec = q - er * OW;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      if (q + reg < P) {
        bf16* dp = dst + ((er + 1) * WS + (ec + 1)) * K + lo;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
          float v = acc[0][ct][reg] + acc[1][ct][reg];
          if (FIRST) {
            float t = (float)(bf16)v + f1[ct];
            dp[ct * 16] = (bf16)(t > 0.f ? t : 0.f);
          } else {
            v += f1[ct] + f2[ct] + (float)dp[ct * 16];
            dp[ct * 16] = (bf16)v;
          }
        }
      }
      if (++ec == OW) {
        ec = 0;
        ++er;
      }
    }
  }
}

constexpr int threadsFor(int K) { return K == 16 ? 1024 : 512; }

template <int K>
__global__ __launch_bounds__(threadsFor(K)) void actor_section_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) char actorSectionLds[];
  constexpr int C8 = K / 8;
  const int n = blockIdx.x;
  const int H = a.H, W = a.W, OH = a.OH, OW = a.OW;
  const int WS = OW + 2;
  const int imgElems = (OH + 2) * WS * K;
  bf16* A = reinterpret_cast<bf16*>(actorSectionLds);
  bf16* B = A + imgElems;

  for (int i = threadIdx.x; i < 2 * imgElems / 8; i += blockDim.x)
    reinterpret_cast<bf16x8*>(A)[i] = zero8();
  __syncthreads();

  // ---- pool: maxpool3x3s2_fwd_kernel's scan, NaN rule included ----
  const int chunks = OH * OW * C8;
  const bf16* un = a.u + (int64_t)n * H * W * K;
  for (int idx = threadIdx.x; idx < chunks; idx += blockDim.x) {
    const int c8 = idx % C8;
    const int t = idx / C8;
    const int ow = t % OW, oh = t / OW;
    float best[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) best[j] = -INFINITY;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int ih = oh * 2 - 1 + kh;
      if (ih < 0 || ih >= H) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int iw = ow * 2 - 1 + kw;
        if (iw < 0 || iw >= W) continue;
        const bf16x8 vin =
            *reinterpret_cast<const bf16x8*>(un + ((int64_t)ih * W + iw) * K + c8 * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float v = (float)vin[j];
          if (v > best[j] || v != v) best[j] = v;
        }
      }
    }
    bf16x8 vout;
#pragma unroll
    for (int j = 0; j < 8; ++j) vout[j] = (bf16)best[j];
    *reinterpret_cast<bf16x8*>(A + ((oh + 1) * WS + (ow + 1)) * K + c8 * 8) = vout;
  }
  __syncthreads();

  conv_pass<K, true>(A, B, a.w[0], a.pending, a.b[0], nullptr, OH, OW);
  __syncthreads();
  conv_pass<K, false>(B, A, a.w[1], nullptr, a.b[1], a.pending, OH, OW);
  __syncthreads();
  conv_pass<K, true>(A, B, a.w[2], nullptr, a.b[2], nullptr, OH, OW);
  __syncthreads();
  conv_pass<K, false>(B, A, a.w[3], nullptr, a.b[3], nullptr, OH, OW);
  __syncthreads();

  bf16* on = a.out + (int64_t)n * OH * OW * K;
  for (int idx = threadIdx.x; idx < chunks; idx += blockDim.x) {
    const int c8 = idx % C8;
    const int t = idx / C8;
    const int ow = t % OW, oh = t / OW;
    bf16x8 v = *reinterpret_cast<const bf16x8*>(A + ((oh + 1) * WS + (ow + 1)) * K + c8 * 8);
    if (a.reluOut) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = (float)v[e];
        v[e] = (bf16)(f > 0.f ? f : 0.f);
      }
    }
    *reinterpret_cast<bf16x8*>(on + (int64_t)idx * 8) = v;
  }
}

inline int64_t ldsBytes(int64_t K, int64_t H, int64_t W) {
  return 2 * ((H + 1) / 2 + 2) * ((W + 1) / 2 + 2) * K * (int64_t)sizeof(bf16);
}

}  // namespace actor_section

at::Tensor actor_section_nhwc(at::Tensor u, c10::optional<at::Tensor> pendingBias,
                              std::vector<at::Tensor> packs, std::vector<at::Tensor> biases,
                              bool reluOut) {
  namespace as = actor_section;
  TORCH_CHECK(u.is_cuda() && u.dim() == 4 && u.scalar_type() == at::kBFloat16,
              "actor_section: bf16 4D CUDA tensor expected");
  TORCH_CHECK(u.is_contiguous(at::MemoryFormat::ChannelsLast),
              "actor_section: channels_last expected");
  const int64_t N = u.size(0), K = u.size(1), H = u.size(2), W = u.size(3);
  TORCH_CHECK(K == 16 || K == 32, "actor_section: K in {16,32}");
  TORCH_CHECK(H >= 1 && W >= 1 && N <= INT_MAX, "actor_section: empty image or too many images");
  TORCH_CHECK(packs.size() == 4 && biases.size() == 4,
              "actor_section: four packs and four biases expected");
  // The kernel indexes every operand from K and the image shape alone: reject
  // anything it would read out of range or reinterpret.
  auto checkVec = [&](const at::Tensor& t, int64_t n, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == u.device() && t.scalar_type() == at::kBFloat16 &&
                    t.is_contiguous(),
                "actor_section: ", name, " must be a contiguous bf16 tensor on u's device");
    TORCH_CHECK(t.numel() == n, "actor_section: ", name, " has ", t.numel(),
                " elements, expected ", n);
  };
  for (int i = 0; i < 4; ++i) {
    checkVec(packs[i], (int64_t)((9 * K + 31) / 32) * 32 * K, "w_packed");
    checkVec(biases[i], K, "bias");
  }
  if (pendingBias.has_value()) checkVec(*pendingBias, K, "pending_bias");

  int ldsDevice = 0;
  TORCH_CHECK(hipDeviceGetAttribute(&ldsDevice, hipDeviceAttributeMaxSharedMemoryPerBlock,
                                    u.get_device()) == hipSuccess,
              "actor_section: cannot query the device's LDS size");
  const int64_t lds = as::ldsBytes(K, H, W);
  TORCH_CHECK(lds <= std::min<int64_t>(as::kLdsMax, ldsDevice), "actor_section: two pooled ",
              (H + 1) / 2, "x", (W + 1) / 2, "x", K, " images need ", lds,
              " bytes of LDS, the workgroup has ", std::min<int64_t>(as::kLdsMax, ldsDevice));

  const int OH = (int)((H + 1) / 2), OW = (int)((W + 1) / 2);
  auto out = at::empty({N, K, OH, OW}, u.options().memory_format(at::MemoryFormat::ChannelsLast));
  if (N == 0) return out;

  as::Args a;
  a.u = reinterpret_cast<const as::bf16*>(u.data_ptr());
  a.pending = pendingBias.has_value()
                  ? reinterpret_cast<const as::bf16*>(pendingBias->data_ptr())
                  : nullptr;
  for (int i = 0; i < 4; ++i) {
    a.w[i] = reinterpret_cast<const as::bf16*>(packs[i].data_ptr());
    a.b[i] = reinterpret_cast<const as::bf16*>(biases[i].data_ptr());
  }
  a.out = reinterpret_cast<as::bf16*>(out.data_ptr());
  a.H = (int)H;
  a.W = (int)W;
  a.OH = OH;
  a.OW = OW;
  a.reluOut = reluOut ? 1 : 0;

  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  // More than 64 KB of dynamic LDS has to be allowed per kernel, once.
  static const bool ldsAllowed = []() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&as::actor_section_kernel<16>),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)as::kLdsMax) == hipSuccess &&
           hipFuncSetAttribute(reinterpret_cast<const void*>(&as::actor_section_kernel<32>),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)as::kLdsMax) == hipSuccess;
  }();
  TORCH_CHECK(ldsAllowed, "actor_section: the runtime refused ", as::kLdsMax,
              " bytes of dynamic LDS");
  if (K == 16) {
    hipLaunchKernelGGL(as::actor_section_kernel<16>, dim3((unsigned)N), dim3(as::threadsFor(16)),
                       (size_t)lds, stream, a);
  } else {
    hipLaunchKernelGGL(as::actor_section_kernel<32>, dim3((unsigned)N), dim3(as::threadsFor(32)),
                       (size_t)lds, stream, a);
  }
  return out;
}
