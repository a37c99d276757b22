// Fused LSTM input projection (gfx950) — included by kernels.hip after
// lstm.hip.inc, whose fragment types and loadAFrag it uses.
//
//   Xg[m, n] = bf16( sum_k feat[m,k] * bf16(W[n,k])                 k < 256
//                    + clamp(reward[m], -1, 1) * bf16(W[n,256])
//                    + bf16(W[n, 257 + a_m])                        0 <= a_m < A
//                    + bias_ih[n] + bias_hh[n] )
//
// W is nn.LSTM's weight_ih_l0, [N = 4H, K = 257 + A], fp32 or bf16, read where
// it lies: no cast copy, no transposed copy, no pack. K is odd-ish (263, 275),
// so a W row starts on a 2- or 4-byte boundary only; every W read is a scalar
// read that runs along the row (a wavefront covers 64 consecutive elements),
// and LDS turns that into the 16-byte fragment reads the MFMA wants.
// An action outside [0, A) selects no column (loadAction returns -1): it
// contributes nothing and is never used as an index.
//
// Four kernels, 256 threads (4 waves) each, mfma_f32_16x16x32_bf16 throughout
// (A: lane holds A[lane&15][(lane>>4)*8 + e]; B: B[(lane>>4)*8 + e][lane&15];
// D: col = lane&15, row = (lane>>4)*4 + reg). Both MFMA operands want 8
// consecutive k per lane, so an operand whose k axis is its slow axis in
// memory goes through LDS transposed: a lane packs the values of two
// consecutive k into one dword and writes it to [col][k]; lanes are laid out
// so that, with the 72-element (36-dword) row pitch, the 64 dword writes of a
// wave and the 16-byte fragment reads both hit distinct banks: 16 columns x 4
// k-pairs where the source is read by scalars (W), 2 column octets x 32
// k-pairs where it is read 16 bytes at a time (dXg and feat in wgrad).
//
// fwd (NT product, K = 256 resident): a workgroup owns BM x 64 of Xg. It
//   stages its feat rows (16-byte reads) and its 64 W rows (scalar reads along
//   the row, fp32 -> bf16 on the way) into LDS with pitch 264, the sparse
//   block W[n, 256 : 257+A] as bf16, the summed biases, the clamped rewards
//   and the checked actions. Wave w owns 16 columns: its 8 B fragments stay in
//   registers across the BM/16 row tiles, 8 MFMAs per 16x16 tile. The epilogue
//   adds reward * column, the gathered action column and the bias in the D
//   layout, in fp32, and rounds once.
//   Tile: 64 columns always. BM = 32 below 1024 rows: the actor's M = 128..256
//   at H = 256 gives 64..128 workgroups (16 column tiles x 4..8 row tiles),
//   where BM = 64 would give 32..64 on 256 CUs. BM = 64 from 1024 rows on: at
//   M = 5120, H = 512 that is 80 x 32 workgroups, and the W tile (64 KB as
//   fp32) is re-read 80 times instead of 160, from L2. The row tile is the
//   fast grid axis, so workgroups that run together share their W tile.
// dgrad: d_feat[M, 256] = dXg[M, N] @ W[:, :256]. A workgroup owns BM rows x
//   64 feature columns (grid: row tiles x 4) and loops over N in chunks of 64
//   with double-buffered LDS: chunk c+1 is fetched into registers before the
//   MFMAs of chunk c and written to the other buffer after them, one barrier
//   per chunk. dXg is k-contiguous; W[n][j] is not and is transposed as above.
// wgrad: [dW_ih | db] = dXg^T @ Z, Z[m] = [feat[m] | clamp(r_m) | onehot(a_m) | 1].
//   A workgroup owns 64 rows n, all 258 + A columns (padded to whole 16-column
//   tiles, at most 320) and a slab of 512 rows of M, in chunks of 64 with the
//   same double buffering; both operands are transposed through LDS. The
//   A + 2 extra columns are synthesised in LDS from reward / prev_action and
//   never exist in global memory. The reward column is the exception to the
//   MFMA: as a bf16 operand the reward would be rounded, so its column is
//   accumulated in fp32 on the VALU from the same LDS tile (16 FMAs per thread
//   and chunk) and the MFMA sees zeros there. Grid: N/64 x ceil(M/512), 32 x
//   10 at the R2D2 learner's shape. Each workgroup writes its fp32 partial
//   tile to a workspace [slabs, N, padded columns].
// wgrad_reduce: sums the slabs in index order, one thread per output element,
//   and writes dW_ih [N, K] and db [N]. No atomics anywhere: two runs agree
//   bit for bit.

namespace lstm_input {

using lstm::bf16;
using lstm::bf16x8;
using lstm::floatx4;
using lstm::loadAFrag;

constexpr int kThreads = 256;
constexpr int kF = 256;                     // feature width == threads: one W element each
constexpr int kFPad = kF + 8;
constexpr int kMaxExtra = 64;               // reward + A action columns + ones column
constexpr int kMaxActions = kMaxExtra - 2;
constexpr int kBN = 64;                     // Xg columns (W rows) per workgroup
constexpr int kKC = 64;                     // reduction chunk of dgrad and wgrad
constexpr int kKCPad = kKC + 8;
constexpr int kSlab = 512;                  // rows of M per wgrad workgroup
static_assert(kThreads == kF, "W staging reads one element per thread and row");

// dtype tags of the operands that may come in more than one type
enum RealKind { kRealF32, kRealBF16, kRealF16, kRealF64 };
enum IntKind { kIntU8, kIntI8, kIntI16, kIntI32, kIntI64 };

DEV_INLINE float loadReal(const void* p, int kind, int64_t i) {
  switch (kind) {
    case kRealBF16: return (float)static_cast<const bf16*>(p)[i];
    case kRealF16: return (float)static_cast<const _Float16*>(p)[i];
    case kRealF64: return (float)static_cast<const double*>(p)[i];
    default: return static_cast<const float*>(p)[i];
  }
}

// the action as an index into the A action columns, or -1 when it selects none
DEV_INLINE int loadAction(const void* p, int kind, int64_t i, int A) {
  int64_t a;
  switch (kind) {
    case kIntU8: a = static_cast<const uint8_t*>(p)[i]; break;
    case kIntI8: a = static_cast<const int8_t*>(p)[i]; break;
    case kIntI16: a = static_cast<const int16_t*>(p)[i]; break;
    case kIntI32: a = static_cast<const int32_t*>(p)[i]; break;
    default: a = static_cast<const int64_t*>(p)[i]; break;
  }
  return (a >= 0 && a < A) ? (int)a : -1;
}

// NaN stays NaN, as torch.clamp keeps it
DEV_INLINE float clampReward(float r) { return r < -1.f ? -1.f : (r > 1.f ? 1.f : r); }

// two bf16 as one dword, `lo` at the lower address
DEV_INLINE uint32_t pack2(bf16 lo, bf16 hi) {
  return (uint32_t)__builtin_bit_cast(uint16_t, lo) |
         ((uint32_t)__builtin_bit_cast(uint16_t, hi) << 16);
}

DEV_INLINE bf16x8 zeroFrag() {
  bf16x8 z;
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = (bf16)0.f;
  return z;
}

struct RowInputs {
  const void* reward;  // [M]
  const void* action;  // [M]
  int rewardKind, actionKind;
};

// ------------------------------------------------------------------ forward
template <typename WT, int RT>
__global__ __launch_bounds__(kThreads) void fwd_kernel(
    const bf16* __restrict__ feat,  // [M, 256]
    RowInputs rows,
    const WT* __restrict__ W,       // [N, K = 257 + A]
    const void* __restrict__ biasIh, const void* __restrict__ biasHh, int biasKind,  // [N]
    bf16* __restrict__ Xg,          // [M, N]
    int M, int N, int A) {
  constexpr int BM = RT * 16;
  __shared__ __attribute__((aligned(16))) bf16 sA[BM][kFPad];
  __shared__ __attribute__((aligned(16))) bf16 sW[kBN][kFPad];
  // [n][0] the reward column, [n][1 + a] action a; the odd dword pitch keeps
  // the epilogue's reads (16 rows n at once) on distinct banks
  __shared__ bf16 sE[kBN][kMaxExtra + 2];
  __shared__ float sBias[kBN];
  __shared__ float sR[BM];
  __shared__ int sAct[BM];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * kBN;
  const int K = kF + 1 + A;
  const WT* wrow = W + (int64_t)n0 * K;

  for (int i = tid; i < BM * (kF / 8); i += kThreads) {
    const int r = i >> 5, c = (i & 31) * 8;
    bf16x8 v = zeroFrag();
    if (m0 + r < M) v = *reinterpret_cast<const bf16x8*>(feat + (int64_t)(m0 + r) * kF + c);
    *reinterpret_cast<bf16x8*>(&sA[r][c]) = v;
  }
#pragma unroll 8
  for (int r = 0; r < kBN; ++r) sW[r][tid] = (bf16)wrow[(int64_t)r * K + tid];
  for (int i = tid; i < kBN * (A + 1); i += kThreads) {
    const int n = i / (A + 1), e = i - n * (A + 1);
    sE[n][e] = (bf16)wrow[(int64_t)n * K + kF + e];
  }
  if (tid < kBN)
    sBias[tid] = loadReal(biasIh, biasKind, n0 + tid) + loadReal(biasHh, biasKind, n0 + tid);
  if (tid < BM) {
    const int m = m0 + tid;
    const bool ok = m < M;
    sR[tid] = ok ? clampReward(loadReal(rows.reward, rows.rewardKind, m)) : 0.f;
    sAct[tid] = ok ? loadAction(rows.action, rows.actionKind, m, A) : -1;
  }
  __syncthreads();

  bf16x8 b[kF / 32];
#pragma unroll
  for (int kk = 0; kk < kF / 32; ++kk) b[kk] = loadAFrag<kFPad>(sW, wave * 16, kk * 32, lane);
  const int col = wave * 16 + (lane & 15);
  const float wr = (float)sE[col][0];
  const float bias = sBias[col];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    floatx4 acc = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < kF / 32; ++kk) {
      const bf16x8 a = loadAFrag<kFPad>(sA, rt * 16, kk * 32, lane);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[kk], acc, 0, 0, 0);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = rt * 16 + (lane >> 4) * 4 + reg;
      if (m0 + row < M) {
        const int a = sAct[row];
        const float wa = a >= 0 ? (float)sE[col][1 + a] : 0.f;
        const float v = acc[reg] + sR[row] * wr + wa + bias;
        Xg[(int64_t)(m0 + row) * N + n0 + col] = (bf16)v;
      }
    }
  }
}

// ----------------------------------------------------------- input gradient
template <typename WT, int RT>
__global__ __launch_bounds__(kThreads) void dgrad_kernel(
    const bf16* __restrict__ dXg,  // [M, N]
    const WT* __restrict__ W,      // [N, K]
    bf16* __restrict__ dFeat,      // [M, 256]
    int M, int N, int K) {
  constexpr int BM = RT * 16;
  constexpr int kDV = BM * (kKC / 8) / kThreads;  // 16-byte dXg reads per thread and chunk
  static_assert(kDV >= 1, "row tile too small for the staging pattern");
  __shared__ __attribute__((aligned(16))) bf16 sD[2][BM][kKCPad];    // dXg chunk [m][n]
  __shared__ __attribute__((aligned(16))) bf16 sWt[2][kBN][kKCPad];  // W chunk [j][n]

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.x * BM, j0 = blockIdx.y * kBN;
  const int nChunks = N / kKC;

  bf16x8 preD[kDV];
  uint32_t preW[8];
  auto fetch = [&](int c) {
#pragma unroll
    for (int v = 0; v < kDV; ++v) {
      const int i = tid + v * kThreads, r = i >> 3, cc = (i & 7) * 8;
      preD[v] = zeroFrag();
      if (m0 + r < M)
        preD[v] = *reinterpret_cast<const bf16x8*>(dXg + (int64_t)(m0 + r) * N + c * kKC + cc);
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int u = it * 4 + wave, jg = u & 3, pg = u >> 2;
      const int j = j0 + jg * 16 + (lane & 15);
      const int n = c * kKC + (pg * 4 + (lane >> 4)) * 2;
      const WT* p = W + (int64_t)n * K + j;
      preW[it] = pack2((bf16)p[0], (bf16)p[K]);
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int v = 0; v < kDV; ++v) {
      const int i = tid + v * kThreads, r = i >> 3, cc = (i & 7) * 8;
      *reinterpret_cast<bf16x8*>(&sD[buf][r][cc]) = preD[v];
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int u = it * 4 + wave, jg = u & 3, pg = u >> 2;
      *reinterpret_cast<uint32_t*>(&sWt[buf][jg * 16 + (lane & 15)][(pg * 4 + (lane >> 4)) * 2]) =
          preW[it];
    }
  };

  floatx4 acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = floatx4{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  stage(0);
  __syncthreads();
  for (int c = 0; c < nChunks; ++c) {
    const int buf = c & 1;
    if (c + 1 < nChunks) fetch(c + 1);
#pragma unroll
    for (int kk = 0; kk < kKC / 32; ++kk) {
      const bf16x8 b = loadAFrag<kKCPad>(sWt[buf], wave * 16, kk * 32, lane);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const bf16x8 a = loadAFrag<kKCPad>(sD[buf], rt * 16, kk * 32, lane);
        acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[rt], 0, 0, 0);
      }
    }
    if (c + 1 < nChunks) stage(buf ^ 1);
    // the only barrier of the chunk: buffer buf^1 is complete before chunk c+1
    // reads it, and was last read in chunk c-1, before the previous barrier
    __syncthreads();
  }

  const int col = j0 + wave * 16 + (lane & 15);
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = m0 + rt * 16 + (lane >> 4) * 4 + reg;
      if (row < M) dFeat[(int64_t)row * kF + col] = (bf16)acc[rt][reg];
    }
}

// ------------------------------------------------- weight and bias gradient
__global__ __launch_bounds__(kThreads) void wgrad_kernel(
    const bf16* __restrict__ dXg,   // [M, N]
    const bf16* __restrict__ feat,  // [M, 256]
    RowInputs rows,
    float* __restrict__ ws,         // [slabs, N, nCT * 16] partial [dW | db | padding]
    int M, int N, int A, int nCT) {
  constexpr int kMaxCT = (kF + kMaxExtra) / 16;  // 20 column tiles at most
  constexpr int kWaveCT = kMaxCT / 4;            // column tiles per wave: w, w+4, ...
  constexpr int kRT = kBN / 16;
  __shared__ __attribute__((aligned(16))) bf16 sGt[2][kBN][kKCPad];             // dXg chunk [n][m]
  __shared__ __attribute__((aligned(16))) bf16 sZt[2][kF + kMaxExtra][kKCPad];  // Z chunk [c][m]
  __shared__ float sR[2][kKC];
  __shared__ float sRed[4][kBN];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n0 = blockIdx.x * kBN;
  const int ms = blockIdx.y * kSlab;
  const int slabRows = min(kSlab, M - ms);
  const int nChunks = (slabRows + kKC - 1) / kKC;
  const int nExtraIt = (nCT - kF / 16) * 2;  // 256 extra-column dwords per pass, 8 columns each

  uint32_t preG[8], preZ[32], preX[8];
  float preR = 0.f;
  auto fetch = [&](int c) {
    const int mb = ms + c * kKC;
    const int mp2 = mb + (lane & 31) * 2;  // this lane's row pair: mp2, mp2 + 1
    // rows m, m+1 of 8 consecutive columns per lane, as two 16-byte reads
    auto rowPair = [&](const bf16* base, int pitch, int col, uint32_t* pre) {
      const bf16* p = base + (int64_t)mp2 * pitch + col;
      const bf16x8 x0 = mp2 < M ? *reinterpret_cast<const bf16x8*>(p) : zeroFrag();
      const bf16x8 x1 = mp2 + 1 < M ? *reinterpret_cast<const bf16x8*>(p + pitch) : zeroFrag();
#pragma unroll
      for (int i = 0; i < 8; ++i) pre[i] = pack2(x0[i], x1[i]);
    };
    rowPair(dXg, N, n0 + wave * 16 + (lane >> 5) * 8, preG);
#pragma unroll
    for (int it = 0; it < 4; ++it)
      rowPair(feat, kF, (it * 4 + wave) * 16 + (lane >> 5) * 8, preZ + it * 8);
    // extra column e: 0 reward (zeros here, see the header), 1..A the one-hot
    // action, A+1 ones, zeros beyond; rows past M are zero in every column
    const int a0 = mp2 < M ? loadAction(rows.action, rows.actionKind, mp2, A) : -1;
    const int a1 = mp2 + 1 < M ? loadAction(rows.action, rows.actionKind, mp2 + 1, A) : -1;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int e = (tid >> 5) + it * 8;
      const bool ones = e == A + 1;
      const float z0 = mp2 < M && (ones || (e >= 1 && a0 == e - 1)) ? 1.f : 0.f;
      const float z1 = mp2 + 1 < M && (ones || (e >= 1 && a1 == e - 1)) ? 1.f : 0.f;
      preX[it] = pack2((bf16)z0, (bf16)z1);
    }
    if (tid < kKC) {
      const int m = mb + tid;
      preR = m < M ? clampReward(loadReal(rows.reward, rows.rewardKind, m)) : 0.f;
    }
  };
  auto stage = [&](int buf) {
    // lane = (8-column half, row pair): the 64 dwords of one store go to
    // banks 32 * half + pair, all distinct
    const int ml = (lane & 31) * 2, c8 = (lane >> 5) * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      *reinterpret_cast<uint32_t*>(&sGt[buf][wave * 16 + c8 + i][ml]) = preG[i];
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
      for (int i = 0; i < 8; ++i)
        *reinterpret_cast<uint32_t*>(&sZt[buf][(it * 4 + wave) * 16 + c8 + i][ml]) =
            preZ[it * 8 + i];
#pragma unroll
    for (int it = 0; it < 8; ++it)
      if (it < nExtraIt)
        *reinterpret_cast<uint32_t*>(&sZt[buf][kF + (tid >> 5) + it * 8][(tid & 31) * 2]) =
            preX[it];
    if (tid < kKC) sR[buf][tid] = preR;
  };

  floatx4 acc[kWaveCT][kRT];
#pragma unroll
  for (int i = 0; i < kWaveCT; ++i)
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt) acc[i][rt] = floatx4{0.f, 0.f, 0.f, 0.f};
  float racc = 0.f;  // reward column, row n = tid & 63, rows m = wave*16 .. +15 of each chunk

  fetch(0);
  stage(0);
  __syncthreads();
  for (int c = 0; c < nChunks; ++c) {
    const int buf = c & 1;
    if (c + 1 < nChunks) fetch(c + 1);
#pragma unroll
    for (int kk = 0; kk < kKC / 32; ++kk) {
      bf16x8 a[kRT];
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt) a[rt] = loadAFrag<kKCPad>(sGt[buf], rt * 16, kk * 32, lane);
#pragma unroll
      for (int i = 0; i < kWaveCT; ++i) {
        const int ct = wave + 4 * i;
        if (ct < nCT) {
          const bf16x8 b = loadAFrag<kKCPad>(sZt[buf], ct * 16, kk * 32, lane);
#pragma unroll
          for (int rt = 0; rt < kRT; ++rt)
            acc[i][rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[rt], b, acc[i][rt], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int mm = 0; mm < 16; ++mm) {
      const int m = wave * 16 + mm;
      racc = fmaf((float)sGt[buf][tid & 63][m], sR[buf][m], racc);
    }
    if (c + 1 < nChunks) stage(buf ^ 1);
    // one barrier per chunk, as in dgrad_kernel
    __syncthreads();
  }

  const int CW = nCT * 16;
  float* out = ws + ((int64_t)blockIdx.y * N + n0) * CW;
#pragma unroll
  for (int i = 0; i < kWaveCT; ++i) {
    const int ct = wave + 4 * i;
    if (ct < nCT) {
      const int col = ct * 16 + (lane & 15);
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int row = rt * 16 + (lane >> 4) * 4 + reg;
          if (col != kF) out[(int64_t)row * CW + col] = acc[i][rt][reg];
        }
    }
  }
  sRed[wave][tid & 63] = racc;
  __syncthreads();
  if (tid < kBN)
    out[(int64_t)tid * CW + kF] = ((sRed[0][tid] + sRed[1][tid]) + sRed[2][tid]) + sRed[3][tid];
}

__global__ __launch_bounds__(kThreads) void wgrad_reduce_kernel(
    const float* __restrict__ ws,  // [slabs, N, CW]
    float* __restrict__ dW,        // [N, K]
    float* __restrict__ db,        // [N]
    int slabs, int N, int K, int CW) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= (int64_t)N * (K + 1)) return;
  const int n = (int)(idx / (K + 1)), c = (int)(idx - (int64_t)n * (K + 1));
  float s = 0.f;
  for (int sl = 0; sl < slabs; ++sl) s += ws[((int64_t)sl * N + n) * CW + c];
  if (c < K)
    dW[(int64_t)n * K + c] = s;
  else
    db[n] = s;
}

}  // namespace lstm_input
