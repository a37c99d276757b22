// Everything that touches weight_hh_l0 outside the scan (gfx950) — included by
// kernels.hip after lstm_input.hip.inc, whose pack2 / zeroFrag and whose LDS
// transposition pattern it uses.
//
// grad: the recurrent weight gradient of the masked LSTM scan,
//
//   dW[n, j] = sum_{m < M = T*B} dG[m, n] * Hp[m, j]                n < 4H, j < H
//   Hp[m]    = notdone[m] != 0 ? (m < B ? h0[m] : H[m - B]) : 0
//
//   dG [M, 4H], H [M, H] and h0 [B, H] are bf16, notdone [M] fp32, dW fp32. In
//   the flattened row index the shift by one time step is an offset of B rows,
//   so Hp never exists in memory: a lane that fetches row m of the H operand
//   reads notdone[m], then h0 + m*H or H + (m-B)*H, or nothing at all when the
//   row is masked (selected to zero, not multiplied). H is a multiple of 8, so
//   every row start is 16-byte aligned for both operands whatever B is. The
//   row indices a lane dereferences are m in [slab start, min(slab end, M))
//   for dG and notdone, m in [0, B) for h0 and m - B in [0, M - B) for H; rows
//   at or past M are zeros in both operands.
//
//   m is the slow axis of both operands and mfma_f32_16x16x32_bf16 wants 8
//   consecutive k per lane from each (A: A[lane&15][(lane>>4)*8 + e], B:
//   B[(lane>>4)*8 + e][lane&15], D: col = lane&15, row = (lane>>4)*4 + reg),
//   so both go through LDS transposed, as in lstm_input::wgrad_kernel: a lane
//   owns a row pair (m, m+1) and 8 consecutive columns, reads them with two
//   16-byte loads, packs the two rows of a column into one dword and writes it
//   to [column][m]. With the 72-element (36-dword) pitch the 64 dword writes
//   of a wave (2 column octets x 32 row pairs: banks 32*octet + pair) and the
//   16-byte fragment reads are conflict-free. One LDS array holds the TN dG
//   columns followed by the TJ H columns of the tile; a pass of the 256
//   threads moves 64 of those columns, wave w taking octets 2w and 2w+1.
//   Chunks of 64 rows are double-buffered: chunk c+1 is fetched into registers
//   before the MFMAs of chunk c and written to the other buffer after them,
//   one barrier per chunk. The accumulators stay in registers over the slab.
//
//   Geometry. 4 waves as 2 x 2, a wave owning WM x WN 16x16 tiles, so a
//   workgroup owns TN = 32 WM rows n by TJ = 32 WN columns j, and one slab of
//   5H rows of M (a whole number of chunks). Grid: H/TJ x 4H/TN x slabs,
//   slabs = ceil(M / 5H).
//     H = 512: WM = WN = 2, a 64 x 64 tile (16 accumulator registers per
//       lane, 36 KB of LDS), slab 2560. At the R2D2 learner's M = 5120 that is
//       8 x 32 x 2 = 512 workgroups, two for each of the 256 CUs, so
//       that one's chunk fetch overlaps the other's MFMAs, 40 chunks each.
//       Partials: 2 x 4.2 MB = 8.4 MB against 26.2 MB of operands (21.0 MB dG
//       + 5.2 MB H). A 128 x 128 tile reads LDS least per MFMA but needs four
//       slabs of 1280 to fill the CUs, 16.8 MB of partials written and read
//       once, and breaks the workspace rule below just above one slab. A
//       64 x 128 tile with the same slab (256 workgroups, one per CU) was
//       measured too: 80.3 us against 77.8 us for this one (median device
//       time of kernel plus reduce), so the tile is not what bounds the
//       kernel at this shape; the smaller one is kept.
//     H = 256, 128: WM = WN = 1, a 32 x 32 tile, slab 1280 / 640. At the IMPALA
//       learner's M = 640, H = 256 the operands are 1.6 MB and one partial
//       copy of dW is 1.0 MB, so there is room for one slab only and the
//       grid has to come from the tile: 8 x 32 x 1 = 256 workgroups, 10 chunks
//       each, no workspace. The work is 0.3 GFLOP; a workgroup's time is the
//       latency of its 10 dependent chunk fetches, not its 2 MFMAs per wave and
//       chunk, which is why the smallest tile that still feeds 4 waves wins.
//   Workspace. A single slab writes dW itself: no workspace, no second launch.
//   With s >= 2 slabs M > 5H(s-1), so the operands are more than
//   10H * 5H(s-1) = 50(s-1)H^2 bytes and the partials 16sH^2: never larger.
//   reduce: sums the slabs in index order, four outputs per thread. No atomics
//   anywhere: two runs agree bit for bit.
//
// pack: reads weight_hh_l0 [4H, H] (fp32 or bf16) once and writes both
//   B-fragment layouts of ops/lstm.py pack_mfma_b (fragment (ct, kk) lane l is
//   8 bf16 at ((ct*KK + kk)*64 + l)*8, element e = W[kk*32 + (l>>4)*8 + e]
//   [ct*16 + (l&15)]): packedT from W = w^T (the forward scan) and packedN
//   from W = w (the backward scan). A workgroup rounds a 32 x 32 block of w to
//   bf16 into LDS, once; that block is two whole fragments of each layout, so
//   each of the 256 threads assembles one lane's 8 values (along the LDS row
//   for packedT, down a column for packedN) and writes them with one 16-byte
//   store.

namespace lstm_whh {

using lstm::bf16;
using lstm::bf16x8;
using lstm::floatx4;
using lstm::loadAFrag;
using lstm_input::pack2;
using lstm_input::zeroFrag;

constexpr int kThreads = 256;
constexpr int kKC = 64;  // rows of M per chunk
constexpr int kKCPad = kKC + 8;

template <int H>
struct Geo {
  static constexpr int kWM = H == 512 ? 2 : 1;  // 16x16 tiles per wave along n
  static constexpr int kWN = H == 512 ? 2 : 1;  // and along j
  static constexpr int kTN = 32 * kWM, kTJ = 32 * kWN;
  static constexpr int kSlab = 5 * H;
  static_assert(kSlab % kKC == 0 && (4 * H) % kTN == 0 && H % kTJ == 0, "whole chunks and tiles");
};

template <int WM, int WN>
__global__ __launch_bounds__(kThreads) void grad_kernel(
    const bf16* __restrict__ dG,        // [M, N = 4H]
    const bf16* __restrict__ Hs,        // [M, Hd]; its last B rows are never read
    const bf16* __restrict__ h0,        // [B, Hd]
    const float* __restrict__ notdone,  // [M]
    float* __restrict__ out,            // [slabs, N, Hd]
    int M, int B, int N, int Hd, int slab) {
  constexpr int TN = 32 * WM, TJ = 32 * WN;
  constexpr int kPasses = (TN + TJ) / 64;  // 8 column octets per pass
  static_assert((TN + TJ) % 64 == 0, "a pass stages 64 columns");
  // rows [0, TN): dG columns n0.. as [n][m]; rows [TN, TN + TJ): Hp columns j0.. as [j][m]
  __shared__ __attribute__((aligned(16))) bf16 sT[2][TN + TJ][kKCPad];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int j0 = blockIdx.x * TJ, n0 = blockIdx.y * TN;
  const int ms = blockIdx.z * slab;
  const int mEnd = min(ms + slab, M);
  const int nChunks = (mEnd - ms + kKC - 1) / kKC;

  uint32_t pre[kPasses][8];
  auto fetch = [&](int c) {
    const int m = ms + c * kKC + (lane & 31) * 2;  // this lane's row pair: m, m + 1
    const bool in0 = m < mEnd, in1 = m + 1 < mEnd;
    const bool live0 = in0 && notdone[m] != 0.f, live1 = in1 && notdone[m + 1] != 0.f;
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
      const int o = p * 8 + wave * 2 + (lane >> 5);  // column octet; dG or Hp per wave
      bf16x8 x0 = zeroFrag(), x1 = zeroFrag();
      if (o < TN / 8) {
        const bf16* g = dG + (int64_t)m * N + n0 + o * 8;
        if (in0) x0 = *reinterpret_cast<const bf16x8*>(g);
        if (in1) x1 = *reinterpret_cast<const bf16x8*>(g + N);
      } else {
        // the step before row r: h0 for the first B rows, H shifted by B after
        auto prev = [&](int r) {
          return (r < B ? h0 + (int64_t)r * Hd : Hs + (int64_t)(r - B) * Hd) + j0 + o * 8 - TN;
        };
        if (live0) x0 = *reinterpret_cast<const bf16x8*>(prev(m));
        if (live1) x1 = *reinterpret_cast<const bf16x8*>(prev(m + 1));
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) pre[p][i] = pack2(x0[i], x1[i]);
    }
  };
  auto stage = [&](int buf) {
    const int ml = (lane & 31) * 2;
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
      const int o = p * 8 + wave * 2 + (lane >> 5);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        *reinterpret_cast<uint32_t*>(&sT[buf][o * 8 + i][ml]) = pre[p][i];
    }
  };

  const int rowBase = (wave >> 1) * WM * 16, colBase = (wave & 1) * WN * 16;
  floatx4 acc[WM][WN];
#pragma unroll
  for (int rt = 0; rt < WM; ++rt)
#pragma unroll
    for (int ct = 0; ct < WN; ++ct) acc[rt][ct] = floatx4{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  stage(0);
  __syncthreads();
  for (int c = 0; c < nChunks; ++c) {
    const int buf = c & 1;
    if (c + 1 < nChunks) fetch(c + 1);
#pragma unroll
    for (int kk = 0; kk < kKC / 32; ++kk) {
      bf16x8 a[WM];
#pragma unroll
      for (int rt = 0; rt < WM; ++rt)
        a[rt] = loadAFrag<kKCPad>(sT[buf], rowBase + rt * 16, kk * 32, lane);
#pragma unroll
      for (int ct = 0; ct < WN; ++ct) {
        const bf16x8 b = loadAFrag<kKCPad>(sT[buf], TN + colBase + ct * 16, kk * 32, lane);
#pragma unroll
        for (int rt = 0; rt < WM; ++rt)
          acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[rt], b, acc[rt][ct], 0, 0, 0);
      }
    }
    if (c + 1 < nChunks) stage(buf ^ 1);
    // the only barrier of the chunk: buffer buf^1 is complete before chunk c+1
    // reads it, and was last read in chunk c-1, before the previous barrier
    __syncthreads();
  }

  float* tile = out + ((int64_t)blockIdx.z * N + n0 + rowBase) * Hd + j0 + colBase;
#pragma unroll
  for (int rt = 0; rt < WM; ++rt)
#pragma unroll
    for (int ct = 0; ct < WN; ++ct)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = rt * 16 + (lane >> 4) * 4 + reg;
        tile[(int64_t)row * Hd + ct * 16 + (lane & 15)] = acc[rt][ct][reg];
      }
}

__global__ __launch_bounds__(kThreads) void grad_reduce_kernel(
    const float4* __restrict__ ws,  // [slabs, n4]
    float4* __restrict__ dW,        // [n4] = [4H, H] as float4
    int slabs, int n4) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  if (idx >= n4) return;
  float4 s = ws[idx];
  for (int sl = 1; sl < slabs; ++sl) {
    const float4 v = ws[(int64_t)sl * n4 + idx];
    s.x += v.x;
    s.y += v.y;
    s.z += v.z;
    s.w += v.w;
  }
  dW[idx] = s;
}

// ---------------------------------------------------------------- W_hh pack
template <typename WT>
__global__ __launch_bounds__(kThreads) void pack_kernel(
    const WT* __restrict__ w,      // [4H, H]
    bf16* __restrict__ packedT,    // pack_mfma_b(w^T): K = H, N = 4H
    bf16* __restrict__ packedN,    // pack_mfma_b(w):   K = 4H, N = H
    int Hd) {
  __shared__ __attribute__((aligned(16))) bf16 s[32][40];  // 80-byte rows: 16-byte aligned octets
  const int tid = threadIdx.x;
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  {
    const int r = tid >> 3, c = (tid & 7) * 4;
    const WT* p = w + (int64_t)(r0 + r) * Hd + c0 + c;
#pragma unroll
    for (int i = 0; i < 4; ++i) s[r][c + i] = (bf16)p[i];
  }
  __syncthreads();
  const int f = tid >> 6, lane = tid & 63, hi = lane >> 4, lo = lane & 15;
  bf16x8 v;
  bf16* dst;
  if (f < 2) {  // fragment (ct = (r0 + 16 f)/16, kk = c0/32) of w^T: along the row
    v = *reinterpret_cast<const bf16x8*>(&s[f * 16 + lo][hi * 8]);
    dst = packedT + ((int64_t)((r0 / 16 + f) * (Hd / 32) + c0 / 32) * 64 + lane) * 8;
  } else {      // fragment (ct = (c0 + 16 (f-2))/16, kk = r0/32) of w: down the column
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = s[hi * 8 + e][(f - 2) * 16 + lo];
    dst = packedN + ((int64_t)((c0 / 16 + f - 2) * (Hd / 8) + r0 / 32) * 64 + lane) * 8;
  }
  *reinterpret_cast<bf16x8*>(dst) = v;
}

}  // namespace lstm_whh
