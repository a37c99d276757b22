// Fused trunk FC (gfx950) — included by kernels.hip after lstm.hip.inc and
// lstm_input.hip.inc, whose fragment types, loadAFrag, pack2, zeroFrag and
// loadReal it uses.
//
//   feat[m, n] = bf16( relu( sum_{c,p} r(x[m,c,p]) * bf16(W[n, c*P + p]) + b[n] ) )
//   r = relu if reluIn else identity;  C = 32, N = 256, P = Hh*Ww >= 1
//
// x is NHWC: row m is P pixels x 32 contiguous channels, K = 32 P bf16. In that
// order (k' = p*32 + c) one MFMA k-step of mfma_f32_16x16x32_bf16 is exactly
// one pixel and every A-fragment read of x is a plain 16-byte read; reluIn is a
// max on it. W is nn.Linear's [256, C*P] in its own NCHW column order
// (k = c*P + p), fp32 or bf16, read where it lies: for a pixel the 32 channels
// of a W row sit P elements apart. All W reads are scalar reads whose lanes
// run along p (8 consecutive pixels of one (n, c), two c per lane), converted
// to bf16 on the way, packed in pairs and transposed by LDS into what the MFMA
// wants. P = 121 is odd, so no wider W read would be aligned anyway.
//
// All kernels: 256 threads (4 waves), mfma_f32_16x16x32_bf16 (A: lane holds
// A[lane&15][(lane>>4)*8 + e]; B: B[(lane>>4)*8 + e][lane&15]; D: col =
// lane&15, row = (lane>>4)*4 + reg), pixels in chunks of kPC = 8 (k = 256).
//
// LDS banks (64 banks of 4 bytes, as in lstm_input.hip.inc). A 16-byte
// fragment read is served 16 lanes at a time (lanes with one value of
// lane>>4): lane l reads row (l&15) at a fixed offset, so the 16 reads start
// at dword pitchD * (l&15) and cover 4 banks each. They tile all 64 banks
// exactly when pitchD / 4 is odd:
//   forward W tile and x tile [row][256 + 8]: pitchD = 132, 132/4 = 33;
//   dgrad / wgrad transposed tiles [row][64 + 8]: pitchD = 36, 36/4 = 9.
// Writes. Forward W tile [n][p*32 + c]: a wave writes 8 pixels x 8 channel
// pairs of one n as dwords, bank 16 p + cp: 32 banks, a 2-way conflict; it is
// the price of reading W in runs of 8 pixels and not 4 (4 p x 16 cp would be
// conflict-free with half the run length). Not measured either way.
// dgrad W tile [col][n], col = c*8 + p inside the chunk (the column order of
// the product is free, the epilogue restores NHWC): a wave writes 16
// consecutive cols (2 c x 8 p) x 4 n-pairs, bank 36 col + np: 36 col mod 64
// takes the 16 multiples of 4 once each, plus np < 4: all 64 distinct.
// wgrad tiles: the row-pair pattern of lstm_input's wgrad (2 column octets x
// 32 row pairs, bank 32 half + pair plus 36 i: distinct).
//
// fwd (NT product): a workgroup owns BM rows x 64 columns x one slab of pp
//   pixels (grid: row tiles x 4 x S, row tile fastest so that workgroups that
//   run together share their W tile). Per 8-pixel chunk the next x and W
//   chunk is fetched into registers before the MFMAs of this one and staged
//   after them (one LDS buffer, two barriers per chunk: 50 KB of LDS and 182
//   VGPRs at BM = 32, two workgroups per CU). Wave w owns 16 columns: per
//   pixel one B fragment read serves the BM/16 row tiles. With S == 1 the
//   epilogue
//   adds the bias, applies relu and rounds once; otherwise fp32 partials go to
//   ws[S, M, 256] and fwd_reduce sums them in slab order, adds the bias,
//   applies relu and rounds once.
// dgrad: d_x[m, p*32+c] = sum_n dZ[m,n] W[n, c*P+p], dZ = dY * (feat > 0)
//   applied as dY is fetched. A workgroup owns BM rows x 8 pixels (256 output
//   columns; wave w owns 64) and loops over n in 4 chunks of 64 with
//   double-buffered LDS, one barrier per chunk, as lstm_input's dgrad. The
//   epilogue goes through LDS (the dead W buffers) to NHWC order, applies the
//   x > 0 mask of reluIn and stores 16 bytes per lane.
// wgrad: [dW | db] = dZ^T @ [r(x) | 1]. A workgroup owns 64 rows n x 8 pixels
//   (256 columns k') x a slab of 512 rows of M, in chunks of 64 rows, both
//   operands transposed through LDS (row pairs packed into dwords), double
//   buffered. db is summed on the VALU from the dZ tile by the workgroups of
//   pixel chunk 0. fp32 partial tiles go to ws[slabs, 256, 32 P] (k' order)
//   and wsb[slabs, 256].
// wgrad_reduce: a workgroup owns one n and 8 pixels: sums the slabs in index
//   order with coalesced reads in k' order, turns the 8 x 32 tile through LDS
//   and writes dW[n, c*P + p] in nn.Linear's order in runs of 8; db likewise.
// No atomics anywhere and a fixed order of every sum: two runs agree bit for
// bit.
//
// Sizes, and what they rest on. NOT measured against alternatives: kPC = 8,
// the 64-column forward tile, BM and kSlab are carried over from
// lstm_input.hip.inc's reasoning or derived from the grid sizes below. The
// rule for S was written from the grid sizes first and then measured once
// (profiles/trunk_fc_micro.txt, the forced "fused S=" rows): at M = 128 and
// 256 its choice is the fastest or within a quarter of the fastest of S = 1,
// 4, 8, 16; at M = 5120 it is not (S = 1: 229 us with an fp32 W, S = 8: 168 us), so
// a grid of one workgroup per CU is too small a target there. The rule was
// left as written; the file holds every figure. The same file compares the
// kernels with the eager chain: they win the actor's forward and lose the
// captured backward and everything at M = 5120.
//   BM = 32 below 1024 rows, 64 from 1024 on (lstm_input's thresholds): the
//   actor's M = 128..256 gives 4..8 row tiles x 4 column tiles = 16..32
//   workgroups per slab where BM = 64 would give 8..16; at M = 5120, BM = 64
//   halves the times the 4 MB W is re-read (80 instead of 160).
//   S (fcSplit in kernels.hip), from (M, P) alone: the smallest number of
//   whole-chunk slabs that brings the grid to 256 workgroups (one per CU), at
//   most 16. P = 121 is 16 chunks: M = 128 -> 16 x 16 = 256 workgroups of one
//   chunk each; M = 256 -> S = 8; M = 672 (21 row tiles, 84 workgroups) ->
//   S = 4; M = 5120 (BM = 64: 320 workgroups) -> S = 1, no second launch.
//   dgrad grid: row tiles x ceil(P/8): 64 workgroups at M = 128, 1280 at 5120.
//   wgrad grid: 4 x ceil(P/8) x ceil(M/512): 128 at M = 672, 640 at M = 5120.

namespace fc {

using lstm::bf16;
using lstm::bf16x8;
using lstm::floatx4;
using lstm::loadAFrag;
using lstm_input::loadReal;
using lstm_input::pack2;
using lstm_input::zeroFrag;

constexpr int kThreads = 256;
constexpr int kC = 32;                 // channels: one MFMA k-step is one pixel
constexpr int kN = 256;                // fc width
constexpr int kPC = 8;                 // pixels per chunk
constexpr int kKC = kPC * kC;          // 256 k' per chunk
constexpr int kKCPad = kKC + 8;        // forward tiles [row][k']
constexpr int kBN = 64;                // forward columns / wgrad rows n per workgroup
constexpr int kNC = 64;                // reduction chunk of dgrad (n) and wgrad (m)
constexpr int kNCPad = kNC + 8;        // transposed tiles [row][reduction index]
constexpr int kSlab = 512;             // rows of M per wgrad workgroup

DEV_INLINE bf16x8 reluFrag(bf16x8 v) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (float)v[e] > 0.f ? v[e] : (bf16)0.f;
  return v;
}

// a where m > 0, else 0
DEV_INLINE bf16x8 maskFrag(bf16x8 a, bf16x8 m) {
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = (float)m[e] > 0.f ? a[e] : (bf16)0.f;
  return a;
}

// ------------------------------------------------------------------ forward
template <typename WT, int RT>
__global__ __launch_bounds__(kThreads) void fwd_kernel(
    const bf16* __restrict__ x,   // [M, P, 32]
    const WT* __restrict__ W,     // [256, 32 P], column c*P + p
    const void* __restrict__ bias, int biasKind,  // [256]
    bf16* __restrict__ feat,      // [M, 256], written when ws is null
    float* __restrict__ ws,       // [S, M, 256] or null (S == 1)
    int M, int P, int pp, int reluIn) {
  constexpr int BM = RT * 16;
  constexpr int kAV = BM * (kKC / 8) / kThreads;  // 16-byte x reads per thread and chunk
  __shared__ __attribute__((aligned(16))) bf16 sA[BM][kKCPad];
  __shared__ __attribute__((aligned(16))) bf16 sW[kBN][kKCPad];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * kBN;
  const int pBeg = blockIdx.z * pp, pEnd = min(P, pBeg + pp);
  const int nChunks = (pEnd - pBeg + kPC - 1) / kPC;
  const int64_t K = (int64_t)kC * P;

  bf16x8 preA[kAV];
  uint32_t preW[32];
  auto fetch = [&](int c) {
    const int pc0 = pBeg + c * kPC;
#pragma unroll
    for (int v = 0; v < kAV; ++v) {
      const int i = tid + v * kThreads, r = i >> 5, cc = (i & 31) * 8;
      preA[v] = zeroFrag();
      if (m0 + r < M && pc0 + (cc >> 5) < pEnd) {
        preA[v] = *reinterpret_cast<const bf16x8*>(x + (int64_t)(m0 + r) * K + (int64_t)pc0 * kC + cc);
        if (reluIn) preA[v] = reluFrag(preA[v]);
      }
    }
    // wave-iteration u: row n = u >> 1, channel pairs (u & 1) * 8 .. + 7;
    // lane: pixel lane & 7, channel pair lane >> 3
    const int p = pc0 + (lane & 7);
#pragma unroll
    for (int it = 0; it < 32; ++it) {
      const int u = it * 4 + wave, n = u >> 1, cp = (u & 1) * 8 + (lane >> 3);
      uint32_t v = 0;
      if (p < pEnd) {
        const WT* q = W + (int64_t)(n0 + n) * K + (int64_t)(2 * cp) * P + p;
        v = pack2((bf16)q[0], (bf16)q[P]);
      }
      preW[it] = v;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int v = 0; v < kAV; ++v) {
      const int i = tid + v * kThreads, r = i >> 5, cc = (i & 31) * 8;
      *reinterpret_cast<bf16x8*>(&sA[r][cc]) = preA[v];
    }
#pragma unroll
    for (int it = 0; it < 32; ++it) {
      const int u = it * 4 + wave, n = u >> 1, cp = (u & 1) * 8 + (lane >> 3);
      *reinterpret_cast<uint32_t*>(&sW[n][(lane & 7) * kC + 2 * cp]) = preW[it];
    }
  };

  floatx4 acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = floatx4{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  for (int c = 0; c < nChunks; ++c) {
    stage();
    __syncthreads();
    if (c + 1 < nChunks) fetch(c + 1);
    const int np = min(kPC, pEnd - (pBeg + c * kPC));
#pragma unroll
    for (int kk = 0; kk < kPC; ++kk) {
      if (kk < np) {
        const bf16x8 b = loadAFrag<kKCPad>(sW, wave * 16, kk * kC, lane);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          const bf16x8 a = loadAFrag<kKCPad>(sA, rt * 16, kk * kC, lane);
          acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[rt], 0, 0, 0);
        }
      }
    }
    // the tiles are free for the next chunk's stage
    __syncthreads();
  }

  const int col = n0 + wave * 16 + (lane & 15);
  const float b = ws == nullptr ? loadReal(bias, biasKind, col) : 0.f;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = m0 + rt * 16 + (lane >> 4) * 4 + reg;
      if (row < M) {
        if (ws == nullptr)
          feat[(int64_t)row * kN + col] = (bf16)fmaxf(acc[rt][reg] + b, 0.f);
        else
          ws[((int64_t)blockIdx.z * M + row) * kN + col] = acc[rt][reg];
      }
    }
}

// four columns per thread
__global__ __launch_bounds__(kThreads) void fwd_reduce_kernel(
    const float* __restrict__ ws,  // [S, M, 256]
    const void* __restrict__ bias, int biasKind,
    bf16* __restrict__ feat,       // [M, 256]
    int M, int S) {
  const int64_t idx = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
  const int64_t total = (int64_t)M * kN;
  if (idx >= total) return;
  const int n = (int)(idx & (kN - 1));
  floatx4 s = floatx4{0.f, 0.f, 0.f, 0.f};
  for (int sl = 0; sl < S; ++sl) s += *reinterpret_cast<const floatx4*>(ws + sl * total + idx);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    feat[idx + e] = (bf16)fmaxf(s[e] + loadReal(bias, biasKind, n + e), 0.f);
}

// ----------------------------------------------------------- input gradient
template <typename WT, int RT>
__global__ __launch_bounds__(kThreads) void dgrad_kernel(
    const bf16* __restrict__ dY,    // [M, 256]
    const bf16* __restrict__ feat,  // [M, 256], the forward's output: the fc relu's mask
    const WT* __restrict__ W,       // [256, 32 P]
    const bf16* __restrict__ x,     // [M, P, 32], read when reluIn
    bf16* __restrict__ dx,          // [M, P, 32]
    int M, int P, int reluIn) {
  constexpr int BM = RT * 16;
  constexpr int kDV = BM * (kNC / 8) / kThreads;  // 16-byte dY reads per thread and chunk
  constexpr int kOV = BM * (kKC / 8) / kThreads;  // 16-byte stores per thread
  static_assert(kDV >= 1, "row tile too small for the staging pattern");
  static_assert(BM * kKCPad <= 2 * kKC * kNCPad, "the output tile reuses the W buffers");
  __shared__ __attribute__((aligned(16))) bf16 sD[2][BM][kNCPad];    // dZ chunk [m][n]
  __shared__ __attribute__((aligned(16))) bf16 sWt[2][kKC][kNCPad];  // W chunk [c*8 + p][n]

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.x * BM, pc0 = blockIdx.y * kPC;
  const int64_t K = (int64_t)kC * P;
  constexpr int nChunks = kN / kNC;

  bf16x8 preD[kDV];
  uint32_t preW[32];
  auto fetch = [&](int c) {
#pragma unroll
    for (int v = 0; v < kDV; ++v) {
      const int i = tid + v * kThreads, r = i >> 3, cc = (i & 7) * 8;
      preD[v] = zeroFrag();
      if (m0 + r < M) {
        const int64_t o = (int64_t)(m0 + r) * kN + c * kNC + cc;
        preD[v] = maskFrag(*reinterpret_cast<const bf16x8*>(dY + o),
                           *reinterpret_cast<const bf16x8*>(feat + o));
      }
    }
    // wave-iteration u: 16 tile columns (channels 2 cg, 2 cg + 1 x 8 pixels)
    // cg = u & 15, n-pair group u >> 4; lane: column lane & 15, n pair lane >> 4
    const int p = pc0 + (lane & 7);
#pragma unroll
    for (int it = 0; it < 32; ++it) {
      const int u = it * 4 + wave, ch = (u & 15) * 2 + ((lane >> 3) & 1);
      const int n = c * kNC + ((u >> 4) * 4 + (lane >> 4)) * 2;
      uint32_t v = 0;
      if (p < P) {
        const WT* q = W + (int64_t)n * K + (int64_t)ch * P + p;
        v = pack2((bf16)q[0], (bf16)q[K]);
      }
      preW[it] = v;
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int v = 0; v < kDV; ++v) {
      const int i = tid + v * kThreads, r = i >> 3, cc = (i & 7) * 8;
      *reinterpret_cast<bf16x8*>(&sD[buf][r][cc]) = preD[v];
    }
#pragma unroll
    for (int it = 0; it < 32; ++it) {
      const int u = it * 4 + wave;
      *reinterpret_cast<uint32_t*>(
          &sWt[buf][(u & 15) * 16 + (lane & 15)][((u >> 4) * 4 + (lane >> 4)) * 2]) = preW[it];
    }
  };

  floatx4 acc[4][RT];  // wave w owns tile columns w*64 .. +63
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[ct][rt] = floatx4{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  stage(0);
  __syncthreads();
  for (int c = 0; c < nChunks; ++c) {
    const int buf = c & 1;
    if (c + 1 < nChunks) fetch(c + 1);
#pragma unroll
    for (int kk = 0; kk < kNC / 32; ++kk) {
      bf16x8 a[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) a[rt] = loadAFrag<kNCPad>(sD[buf], rt * 16, kk * 32, lane);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const bf16x8 b = loadAFrag<kNCPad>(sWt[buf], wave * 64 + ct * 16, kk * 32, lane);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
          acc[ct][rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[rt], b, acc[ct][rt], 0, 0, 0);
      }
    }
    if (c + 1 < nChunks) stage(buf ^ 1);
    // the only barrier of the chunk, as in lstm_input's dgrad; after the last
    // chunk it frees the W buffers for the output tile
    __syncthreads();
  }

  // tile column j = c*8 + p  ->  NHWC offset p*32 + c
  bf16(*sOut)[kKCPad] = reinterpret_cast<bf16(*)[kKCPad]>(&sWt[0][0][0]);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int j = wave * 64 + ct * 16 + (lane & 15);
    const int o = (j & 7) * kC + (j >> 3);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        sOut[rt * 16 + (lane >> 4) * 4 + reg][o] = (bf16)acc[ct][rt][reg];
  }
  __syncthreads();
#pragma unroll
  for (int v = 0; v < kOV; ++v) {
    const int i = tid + v * kThreads, r = i >> 5, cc = (i & 31) * 8;
    if (m0 + r < M && pc0 + (cc >> 5) < P) {
      const int64_t o = (int64_t)(m0 + r) * K + (int64_t)pc0 * kC + cc;
      bf16x8 d = *reinterpret_cast<const bf16x8*>(&sOut[r][cc]);
      if (reluIn) d = maskFrag(d, *reinterpret_cast<const bf16x8*>(x + o));
      *reinterpret_cast<bf16x8*>(dx + o) = d;
    }
  }
}

// ------------------------------------------------- weight and bias gradient
__global__ __launch_bounds__(kThreads) void wgrad_kernel(
    const bf16* __restrict__ dY,    // [M, 256]
    const bf16* __restrict__ feat,  // [M, 256]
    const bf16* __restrict__ x,     // [M, P, 32]
    float* __restrict__ ws,         // [slabs, 256, 32 P] partial dW, column p*32 + c
    float* __restrict__ wsb,        // [slabs, 256] partial db
    int M, int P, int reluIn) {
  constexpr int kRT = kBN / 16;
  __shared__ __attribute__((aligned(16))) bf16 sGt[2][kBN][kNCPad];  // dZ chunk [n][m]
  __shared__ __attribute__((aligned(16))) bf16 sZt[2][kKC][kNCPad];  // r(x) chunk [k'][m]
  __shared__ float sRed[4][kBN];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n0 = blockIdx.x * kBN, pc0 = blockIdx.y * kPC;
  const int ms = blockIdx.z * kSlab;
  const int slabRows = min(kSlab, M - ms);
  const int nChunks = (slabRows + kNC - 1) / kNC;
  const int64_t K = (int64_t)kC * P;
  const bool withBias = blockIdx.y == 0;

  uint32_t preG[8], preZ[32];
  auto fetch = [&](int c) {
    const int mp2 = ms + c * kNC + (lane & 31) * 2;  // this lane's row pair: mp2, mp2 + 1
    const int half = (lane >> 5) * 8;
    {
      const int64_t o = (int64_t)mp2 * kN + n0 + wave * 16 + half;
      bf16x8 g0 = zeroFrag(), g1 = zeroFrag();
      if (mp2 < M)
        g0 = maskFrag(*reinterpret_cast<const bf16x8*>(dY + o),
                      *reinterpret_cast<const bf16x8*>(feat + o));
      if (mp2 + 1 < M)
        g1 = maskFrag(*reinterpret_cast<const bf16x8*>(dY + o + kN),
                      *reinterpret_cast<const bf16x8*>(feat + o + kN));
#pragma unroll
      for (int i = 0; i < 8; ++i) preG[i] = pack2(g0[i], g1[i]);
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int col = (it * 4 + wave) * 16 + half;  // k' inside the chunk, one pixel per 32
      const bool pix = pc0 + (col >> 5) < P;
      const bf16* q = x + (int64_t)mp2 * K + (int64_t)pc0 * kC + col;
      bf16x8 x0 = zeroFrag(), x1 = zeroFrag();
      if (pix && mp2 < M) x0 = *reinterpret_cast<const bf16x8*>(q);
      if (pix && mp2 + 1 < M) x1 = *reinterpret_cast<const bf16x8*>(q + K);
      if (reluIn) {
        x0 = reluFrag(x0);
        x1 = reluFrag(x1);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) preZ[it * 8 + i] = pack2(x0[i], x1[i]);
    }
  };
  auto stage = [&](int buf) {
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
  };

  floatx4 acc[4][kRT];  // column tiles wave, wave + 4, ...
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt) acc[i][rt] = floatx4{0.f, 0.f, 0.f, 0.f};
  float bacc = 0.f;  // db: row n = tid & 63, rows m = wave*16 .. +15 of each chunk

  fetch(0);
  stage(0);
  __syncthreads();
  for (int c = 0; c < nChunks; ++c) {
    const int buf = c & 1;
    if (c + 1 < nChunks) fetch(c + 1);
#pragma unroll
    for (int kk = 0; kk < kNC / 32; ++kk) {
      bf16x8 a[kRT];
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt) a[rt] = loadAFrag<kNCPad>(sGt[buf], rt * 16, kk * 32, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bf16x8 b = loadAFrag<kNCPad>(sZt[buf], (wave + 4 * i) * 16, kk * 32, lane);
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt)
          acc[i][rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[rt], b, acc[i][rt], 0, 0, 0);
      }
    }
    if (withBias) {
#pragma unroll
      for (int mm = 0; mm < 16; ++mm) bacc += (float)sGt[buf][tid & 63][wave * 16 + mm];
    }
    if (c + 1 < nChunks) stage(buf ^ 1);
    // one barrier per chunk, as in dgrad_kernel
    __syncthreads();
  }

  float* out = ws + ((int64_t)blockIdx.z * kN + n0) * K + (int64_t)pc0 * kC;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int col = (wave + 4 * i) * 16 + (lane & 15);
    if (pc0 + (col >> 5) < P) {
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int row = rt * 16 + (lane >> 4) * 4 + reg;
          out[(int64_t)row * K + col] = acc[i][rt][reg];
        }
    }
  }
  if (withBias) {
    sRed[wave][tid & 63] = bacc;
    __syncthreads();
    if (tid < kBN)
      wsb[(int64_t)blockIdx.z * kN + n0 + tid] =
          ((sRed[0][tid] + sRed[1][tid]) + sRed[2][tid]) + sRed[3][tid];
  }
}

__global__ __launch_bounds__(kThreads) void wgrad_reduce_kernel(
    const float* __restrict__ ws,   // [slabs, 256, 32 P], column p*32 + c
    const float* __restrict__ wsb,  // [slabs, 256]
    float* __restrict__ dW,         // [256, 32 P], column c*P + p
    float* __restrict__ db,         // [256]
    int slabs, int P) {
  __shared__ float sT[kC][kPC + 1];
  const int tid = threadIdx.x;
  const int pc0 = blockIdx.x * kPC, n = blockIdx.y;
  const int64_t K = (int64_t)kC * P;
  {
    const int p = tid >> 5, c = tid & 31;
    float s = 0.f;
    if (pc0 + p < P)
      for (int sl = 0; sl < slabs; ++sl) s += ws[((int64_t)sl * kN + n) * K + (int64_t)pc0 * kC + tid];
    sT[c][p] = s;
  }
  __syncthreads();
  {
    const int c = tid >> 3, p = tid & 7;
    if (pc0 + p < P) dW[(int64_t)n * K + (int64_t)c * P + pc0 + p] = sT[c][p];
  }
  if (blockIdx.x == 0 && tid == 0) {
    float s = 0.f;
    for (int sl = 0; sl < slabs; ++sl) s += wsb[(int64_t)sl * kN + n];
    db[n] = s;
  }
}

}  // namespace fc
