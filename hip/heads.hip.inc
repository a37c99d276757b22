// Fused policy and baseline heads (gfx950) — included by kernels.hip after
// lstm_input.hip.inc, whose RowInputs, loadReal, loadAction, clampReward, pack2
// and zeroFrag it uses.
//
//   out[m, n] = sum_k x[m,k] * bf16(W[n,k])                          k < D
//               + clamp(reward[m], -1, 1) * bf16(W[n,256])           composite
//               + bf16(W[n, 257 + a_m])                 0 <= a_m < A, composite
//               + b[n]
//   W = [Wp; Wb], b = [bp; bb]: logits = out[:, :A], baseline = out[:, A]
//
// Wp [A, K], Wb [1, K], bp [A], bb [1] are nn.Linear's own tensors, fp32 or
// bf16, read where they lie: no cast copy, no transpose, no pack, no cat of
// the two heads. N = A + 1 <= 64 columns in NT <= 4 tiles of 16. Dense mode:
// K = D in {128, 256, 512}. Composite mode: D = 256, K = 257 + A in the model's
// column order (features, reward, actions); K is odd-ish, so every W read is a
// scalar read that runs along the row. An action outside [0, A) selects no
// column (loadAction returns -1) and is never used as an index. Outputs and
// incoming gradients are fp32 and are read and written as they are.
//
// Three kernels, mfma_f32_16x16x32_bf16 throughout (A: lane holds
// A[lane&15][(lane>>4)*8 + e]; B: B[(lane>>4)*8 + e][lane&15]; D: col =
// lane&15, row = (lane>>4)*4 + reg). LDS is dynamic: its size follows A.
//
// fwd: a workgroup owns rows only and all N columns. It stages the whole
//   stacked weight into LDS as bf16 with pitch D + 8 (scalar reads along each
//   row, rows N..16*NT zero), in composite mode also the sparse block
//   W[:, 256:], and the biases, the clamped rewards and the checked actions.
//   x does not go through LDS: each 16-row tile belongs to one wave, whose
//   D/32 A fragments are 16-byte global reads issued before the staging and
//   kept in registers across the NT column tiles. The epilogue adds reward *
//   column, the gathered action column and the bias in the D layout, in fp32,
//   and writes logits[m, a] for a < A and column A to baseline[m].
//   Row tile: one wave (16 rows, 64 threads) per workgroup below 1024 rows:
//   the actor's M = 128..256 gives 8..16 workgroups and the IMPALA learner's
//   672 gives 42, where four waves would give 2..4 and 11; the weight (5 K
//   elements at A = 18, composite) is staged by each from L2. Four waves (64
//   rows) from 1024 rows on: M = 5120 is 80 workgroups and the weight is
//   re-read 80 times instead of 320.
// bwd: one pass over x and the incoming gradients, both products. A workgroup
//   (256 threads) owns a slab of 128 rows in chunks of KC = 64 (32 at D = 512,
//   where two 64-row buffers of Z^T alone are 147 KB), double-buffered: chunk
//   c+1 is fetched into registers before the MFMAs of chunk c and written to
//   the other buffer after them, one barrier per chunk. The gradient chunk
//   dOut[m][n] (bf16 of the fp32 dlogits / dbaseline, zero where either is
//   absent, n padded to a multiple of 32) is kept twice: [m][n] for the input
//   gradient and, packed two rows to a dword, [n][m] for the weight gradient.
//   Input gradient: d_x[chunk, D] = dOut @ W[:, :D], one or two k-steps per
//     tile, written as bf16 chunk by chunk. Deviation from "W transposed
//     through LDS": W^T would take D * 72 * 2 = 72 KB at D = 512 next to the
//     Z^T buffers; its fragments (wave w owns column tiles w, w+4, ...) are
//     instead read once per workgroup straight into registers, 8 scalar reads
//     per fragment, 16 lanes along a W row each.
//   Weight gradient: dW += dOut^T @ Z, Z = [x | onehot(p)], with Z^T in LDS
//     (x rows packed in pairs as in lstm_input::wgrad_kernel) and the one-hot
//     columns synthesised there. The reward column and, as a second deviation,
//     the bias column are accumulated in fp32 on the VALU from the same LDS
//     tile: the reward must not be rounded to bf16, and with A = 63 a ones
//     column would be the 65th extra column and cost a fifth 16-column tile.
//   Each workgroup writes its fp32 partial to ws [slabs, 16*NT, D + Epad + 2]:
//   x columns, Epad one-hot columns, the reward column, the bias column.
// wgrad_reduce: sums the slabs in index order, one thread per output element,
//   and writes the four gradients in nn.Linear's layouts. No atomics anywhere:
//   two runs agree bit for bit.

namespace heads {

using lstm::bf16;
using lstm::bf16x8;
using lstm::floatx4;
using lstm_input::clampReward;
using lstm_input::loadAction;
using lstm_input::loadReal;
using lstm_input::pack2;
using lstm_input::RowInputs;
using lstm_input::zeroFrag;

constexpr int kMaxActions = 63;       // N = A + 1 <= 64: four column tiles
constexpr int kCompositeD = 256;      // feature width of the composite mode
constexpr int kExtraPitch = 66;       // sparse block in LDS: [n][0] reward, [n][1 + a]
constexpr int kBwdThreads = 256;
constexpr int kSlab = 128;            // rows of M per bwd workgroup
constexpr int kLdsMax = 160 * 1024;

DEV_INLINE bf16x8 loadFrag(const bf16* buf, int pitch, int rowBase, int k0, int lane) {
  return *reinterpret_cast<const bf16x8*>(buf + (rowBase + (lane & 15)) * pitch + k0 +
                                          (lane >> 4) * 8);
}

// element [n][k] of the stacked weight [Wp; Wb], zero in the padding rows
template <typename WT>
DEV_INLINE bf16 stackedW(const WT* __restrict__ Wp, const WT* __restrict__ Wb, int n, int k, int A,
                         int K) {
  if (n < A) return (bf16)Wp[(int64_t)n * K + k];
  if (n == A) return (bf16)Wb[k];
  return (bf16)0.f;
}

__host__ __device__ constexpr int fwdLdsBytes(int D, int waves, int A, bool composite) {
  const int Npad = (A + 1 + 15) / 16 * 16;
  return Npad * (D + 8) * 2 + Npad * 4 + waves * 16 * 8 + (composite ? Npad * kExtraPitch * 2 : 0);
}

// ------------------------------------------------------------------ forward
template <typename WT, int D, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void fwd_kernel(
    const bf16* __restrict__ x,  // [M, D]
    RowInputs rows,              // composite mode only
    const WT* __restrict__ Wp,   // [A, K]
    const WT* __restrict__ Wb,   // [1, K]
    const void* __restrict__ bp, const void* __restrict__ bb, int biasKind,  // [A], [1]
    float* __restrict__ logits,    // [M, A]
    float* __restrict__ baseline,  // [M]
    int M, int A, int composite) {
  constexpr int kT = WAVES * 64, BM = WAVES * 16, KK = D / 32, P = D + 8;
  extern __shared__ __attribute__((aligned(16))) char headsLds[];
  const int N = A + 1, NT = (N + 15) >> 4, Npad = NT * 16;
  const int K = composite ? D + 1 + A : D;
  bf16* sW = reinterpret_cast<bf16*>(headsLds);            // [Npad][P]
  float* sBias = reinterpret_cast<float*>(sW + Npad * P);  // [Npad]
  float* sR = sBias + Npad;                                // [BM]
  int* sAct = reinterpret_cast<int*>(sR + BM);             // [BM]
  bf16* sE = reinterpret_cast<bf16*>(sAct + BM);           // [Npad][kExtraPitch], composite

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.x * BM + wave * 16;

  // this wave's x tile, in flight while the weight is staged
  bf16x8 a[KK];
  {
    const int m = m0 + (lane & 15);
    const bf16* p = x + (int64_t)m * D + (lane >> 4) * 8;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk)
      a[kk] = m < M ? *reinterpret_cast<const bf16x8*>(p + kk * 32) : zeroFrag();
  }

  for (int i = tid; i < Npad * D; i += kT) {
    const int n = i / D, k = i - n * D;
    sW[n * P + k] = stackedW(Wp, Wb, n, k, A, K);
  }
  if (composite) {
    for (int i = tid; i < Npad * (A + 1); i += kT) {
      const int n = i / (A + 1), e = i - n * (A + 1);
      sE[n * kExtraPitch + e] = stackedW(Wp, Wb, n, D + e, A, K);
    }
    if (tid < BM) {
      const int m = blockIdx.x * BM + tid;
      const bool ok = m < M;
      sR[tid] = ok ? clampReward(loadReal(rows.reward, rows.rewardKind, m)) : 0.f;
      sAct[tid] = ok ? loadAction(rows.action, rows.actionKind, m, A) : -1;
    }
  }
  if (tid < Npad)
    sBias[tid] = tid < A ? loadReal(bp, biasKind, tid) : (tid == A ? loadReal(bb, biasKind, 0) : 0.f);
  __syncthreads();

  for (int ct = 0; ct < NT; ++ct) {
    floatx4 acc = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KK; ++kk)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[kk], loadFrag(sW, P, ct * 16, kk * 32, lane),
                                                    acc, 0, 0, 0);
    const int col = ct * 16 + (lane & 15);
    if (col >= N) continue;
    const float bias = sBias[col];
    const float wr = composite ? (float)sE[col * kExtraPitch] : 0.f;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int r = wave * 16 + (lane >> 4) * 4 + reg;
      const int m = blockIdx.x * BM + r;
      if (m < M) {
        float v = acc[reg];
        if (composite) {
          const int act = sAct[r];
          const float wa = act >= 0 ? (float)sE[col * kExtraPitch + 1 + act] : 0.f;
          v = v + sR[r] * wr + wa;
        }
        v += bias;
        if (col < A)
          logits[(int64_t)m * A + col] = v;
        else
          baseline[m] = v;
      }
    }
  }
}

// ----------------------------------------------------------------- backward
template <int D>
struct BwdTile {
  static constexpr int KC = D == 512 ? 32 : 64;  // rows of M per chunk
  static constexpr int KCP = KC + 8;
  static constexpr int kMaxE = D == kCompositeD ? 64 : 0;        // one-hot columns, padded
  static constexpr int kWaveCT = ((D + kMaxE) / 16 + 3) / 4;     // wgrad column tiles per wave
  static constexpr int kWaveJT = D / 64;                         // d_x column tiles per wave
  static constexpr int kZIt = (KC / 2) * (D / 8) / kBwdThreads;  // (row pair, 8 columns) items
  static_assert(kSlab % KC == 0 && kZIt >= 1, "chunks tile the slab and fill the workgroup");
};

__host__ __device__ constexpr int bwdLdsBytes(int D, int A, bool composite) {
  const int KC = D == 512 ? 32 : 64, KCP = KC + 8;
  const int Nk = (A + 1 + 31) / 32 * 32;
  const int Epad = composite ? (A + 15) / 16 * 16 : 0;
  return 2 * ((D + Epad) * KCP + Nk * KCP + KC * (Nk + 8)) * 2 + 2 * KC * 4 + 2 * 4 * 64 * 4;
}

template <typename WT, int D>
__global__ __launch_bounds__(kBwdThreads) void bwd_kernel(
    const float* __restrict__ dLogits,  // [M, A] or null
    const float* __restrict__ dBase,    // [M] or null
    const bf16* __restrict__ x,         // [M, D]
    RowInputs rows,                     // composite mode only
    const WT* __restrict__ Wp,          // [A, K]
    const WT* __restrict__ Wb,          // [1, K]
    bf16* __restrict__ dx,              // [M, D] or null
    float* __restrict__ ws,             // [slabs, Npad, D + Epad + 2]
    int M, int A, int composite) {
  using T = BwdTile<D>;
  constexpr int KC = T::KC, KCP = T::KCP;
  extern __shared__ __attribute__((aligned(16))) char headsLds[];
  const int N = A + 1, NT = (N + 15) >> 4, Npad = NT * 16;
  const int NK = (N + 31) >> 5, Nk = NK * 32, GP = Nk + 8;
  const int K = composite ? D + 1 + A : D;
  const int Epad = composite ? ((A + 15) >> 4) * 16 : 0;
  const int ZR = D + Epad, nCT = ZR / 16, CW = ZR + 2;
  bf16* sZt = reinterpret_cast<bf16*>(headsLds);         // [2][ZR][KCP]  Z chunk [c][m]
  bf16* sGt = sZt + 2 * ZR * KCP;                        // [2][Nk][KCP]  dOut chunk [n][m]
  bf16* sG = sGt + 2 * Nk * KCP;                         // [2][KC][GP]   dOut chunk [m][n]
  float* sR = reinterpret_cast<float*>(sG + 2 * KC * GP);  // [2][KC]
  float* sRed = sR + 2 * KC;                             // [2][4][64]

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int ms = blockIdx.x * kSlab;
  const int slabRows = min(kSlab, M - ms);
  const int nChunks = (slabRows + KC - 1) / KC;
  const int nGIt = (KC / 2) * Nk / kBwdThreads;  // (row pair, column) items per thread

  // W^T fragments of this wave's d_x column tiles, for the whole slab
  bf16x8 wf[T::kWaveJT][2];
  if (dx != nullptr) {
#pragma unroll
    for (int i = 0; i < T::kWaveJT; ++i)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e)
          wf[i][ks][e] = stackedW(Wp, Wb, ks * 32 + (lane >> 4) * 8 + e,
                                  (wave + 4 * i) * 16 + (lane & 15), A, K);
  }

  auto gradAt = [&](int m, int n) -> float {
    if (m >= M) return 0.f;
    if (n < A) return dLogits != nullptr ? dLogits[(int64_t)m * A + n] : 0.f;
    if (n == A) return dBase != nullptr ? dBase[m] : 0.f;
    return 0.f;
  };

  uint32_t preZ[T::kZIt * 8], preG[8], preX[8];
  float preR = 0.f;
  auto fetch = [&](int c) {
    const int mb = ms + c * KC;
#pragma unroll
    for (int it = 0; it < T::kZIt; ++it) {
      const int u = tid + it * kBwdThreads, pair = u % (KC / 2), cg = u / (KC / 2);
      const int m = mb + 2 * pair;
      const bf16* p = x + (int64_t)m * D + cg * 8;
      const bf16x8 x0 = m < M ? *reinterpret_cast<const bf16x8*>(p) : zeroFrag();
      const bf16x8 x1 = m + 1 < M ? *reinterpret_cast<const bf16x8*>(p + D) : zeroFrag();
#pragma unroll
      for (int i = 0; i < 8; ++i) preZ[it * 8 + i] = pack2(x0[i], x1[i]);
    }
#pragma unroll
    for (int it = 0; it < 8; ++it)
      if (it < nGIt) {
        const int u = tid + it * kBwdThreads, pair = u / Nk, n = u - pair * Nk;
        const int m = mb + 2 * pair;
        preG[it] = pack2((bf16)gradAt(m, n), (bf16)gradAt(m + 1, n));
      }
    if (composite) {
      // one-hot column a of rows (mp, mp + 1); rows past M are zero in every column
      const int mp = mb + (tid & 31) * 2;
      const int a0 = mp < M ? loadAction(rows.action, rows.actionKind, mp, A) : -1;
      const int a1 = mp + 1 < M ? loadAction(rows.action, rows.actionKind, mp + 1, A) : -1;
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int e = (tid >> 5) + it * 8;
        preX[it] = pack2((bf16)(a0 == e ? 1.f : 0.f), (bf16)(a1 == e ? 1.f : 0.f));
      }
      if (tid < KC) {
        const int m = mb + tid;
        preR = m < M ? clampReward(loadReal(rows.reward, rows.rewardKind, m)) : 0.f;
      }
    }
  };
  auto stage = [&](int buf) {
    bf16* zt = sZt + buf * ZR * KCP;
    bf16* gt = sGt + buf * Nk * KCP;
    bf16* g = sG + buf * KC * GP;
#pragma unroll
    for (int it = 0; it < T::kZIt; ++it) {
      const int u = tid + it * kBwdThreads, pair = u % (KC / 2), cg = u / (KC / 2);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        *reinterpret_cast<uint32_t*>(zt + (cg * 8 + i) * KCP + 2 * pair) = preZ[it * 8 + i];
    }
#pragma unroll
    for (int it = 0; it < 8; ++it)
      if (it < nGIt) {
        const int u = tid + it * kBwdThreads, pair = u / Nk, n = u - pair * Nk;
        *reinterpret_cast<uint32_t*>(gt + n * KCP + 2 * pair) = preG[it];
        g[(2 * pair) * GP + n] = __builtin_bit_cast(bf16, (uint16_t)(preG[it] & 0xffffu));
        g[(2 * pair + 1) * GP + n] = __builtin_bit_cast(bf16, (uint16_t)(preG[it] >> 16));
      }
    if (composite) {
#pragma unroll
      for (int it = 0; it < 8; ++it)
        if (it * 8 < Epad)
          *reinterpret_cast<uint32_t*>(zt + (D + (tid >> 5) + it * 8) * KCP + (tid & 31) * 2) =
              preX[it];
      if (tid < KC) sR[buf * KC + tid] = preR;
    }
  };

  floatx4 acc[T::kWaveCT][4];
#pragma unroll
  for (int i = 0; i < T::kWaveCT; ++i)
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[i][rt] = floatx4{0.f, 0.f, 0.f, 0.f};
  // reward and bias columns, row n = tid & 63, rows m = wave*KC/4 .. of each chunk
  float racc = 0.f, bacc = 0.f;

  fetch(0);
  stage(0);
  __syncthreads();
  for (int c = 0; c < nChunks; ++c) {
    const int buf = c & 1;
    const bf16* zt = sZt + buf * ZR * KCP;
    const bf16* gt = sGt + buf * Nk * KCP;
    const bf16* g = sG + buf * KC * GP;
    if (c + 1 < nChunks) fetch(c + 1);

#pragma unroll
    for (int kk = 0; kk < KC / 32; ++kk) {
      bf16x8 ga[4];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
        ga[rt] = rt < NT ? loadFrag(gt, KCP, rt * 16, kk * 32, lane) : zeroFrag();
#pragma unroll
      for (int i = 0; i < T::kWaveCT; ++i) {
        const int ct = wave + 4 * i;
        if (ct < nCT) {
          const bf16x8 b = loadFrag(zt, KCP, ct * 16, kk * 32, lane);
#pragma unroll
          for (int rt = 0; rt < 4; ++rt)
            if (rt < NT)
              acc[i][rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ga[rt], b, acc[i][rt], 0, 0, 0);
        }
      }
    }

    if (dx != nullptr) {
      const int mb = ms + c * KC;
#pragma unroll
      for (int mt = 0; mt < KC / 16; ++mt) {
        const bf16x8 g0 = loadFrag(g, GP, mt * 16, 0, lane);
        const bf16x8 g1 = NK > 1 ? loadFrag(g, GP, mt * 16, 32, lane) : zeroFrag();
#pragma unroll
        for (int i = 0; i < T::kWaveJT; ++i) {
          floatx4 d = floatx4{0.f, 0.f, 0.f, 0.f};
          d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g0, wf[i][0], d, 0, 0, 0);
          if (NK > 1) d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(g1, wf[i][1], d, 0, 0, 0);
          const int col = (wave + 4 * i) * 16 + (lane & 15);
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int m = mb + mt * 16 + (lane >> 4) * 4 + reg;
            if (m < M) dx[(int64_t)m * D + col] = (bf16)d[reg];
          }
        }
      }
    }

    if ((tid & 63) < Npad) {
#pragma unroll
      for (int mm = 0; mm < KC / 4; ++mm) {
        const int m = wave * (KC / 4) + mm;
        const float gv = (float)gt[(tid & 63) * KCP + m];
        bacc += gv;
        if (composite) racc = fmaf(gv, sR[buf * KC + m], racc);
      }
    }

    if (c + 1 < nChunks) stage(buf ^ 1);
    // the only barrier of the chunk: buffer buf^1 is complete before chunk c+1
    // reads it, and was last read in chunk c-1, before the previous barrier
    __syncthreads();
  }

  float* out = ws + (int64_t)blockIdx.x * Npad * CW;
#pragma unroll
  for (int i = 0; i < T::kWaveCT; ++i) {
    const int ct = wave + 4 * i;
    if (ct < nCT) {
      const int col = ct * 16 + (lane & 15);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
        if (rt < NT) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg)
            out[(rt * 16 + (lane >> 4) * 4 + reg) * CW + col] = acc[i][rt][reg];
        }
    }
  }
  sRed[wave * 64 + (tid & 63)] = racc;
  sRed[256 + wave * 64 + (tid & 63)] = bacc;
  __syncthreads();
  if (tid < Npad) {
    out[tid * CW + ZR] = ((sRed[tid] + sRed[64 + tid]) + sRed[128 + tid]) + sRed[192 + tid];
    out[tid * CW + ZR + 1] =
        ((sRed[256 + tid] + sRed[320 + tid]) + sRed[384 + tid]) + sRed[448 + tid];
  }
}

__global__ __launch_bounds__(kBwdThreads) void wgrad_reduce_kernel(
    const float* __restrict__ ws,  // [slabs, Npad, CW]
    float* __restrict__ dWp,       // [A, K]
    float* __restrict__ dbp,       // [A]
    float* __restrict__ dWb,       // [1, K]
    float* __restrict__ dbb,       // [1]
    int slabs, int A, int K, int D, int Npad, int CW) {
  const int idx = blockIdx.x * kBwdThreads + threadIdx.x;
  if (idx >= (A + 1) * (K + 1)) return;
  const int n = idx / (K + 1), c = idx - n * (K + 1);
  // W column c in the workspace: x columns, then (composite) the reward column
  // at CW - 2 and action a at D + a; the bias at CW - 1
  const int wc = c == K ? CW - 1 : (c < D ? c : (c == D ? CW - 2 : c - 1));
  float s = 0.f;
  for (int sl = 0; sl < slabs; ++sl) s += ws[((int64_t)sl * Npad + n) * CW + wc];
  if (n < A) {
    if (c < K)
      dWp[(int64_t)n * K + c] = s;
    else
      dbp[n] = s;
  } else {
    if (c < K)
      dWb[c] = s;
    else
      dbb[0] = s;
  }
}

}  // namespace heads
