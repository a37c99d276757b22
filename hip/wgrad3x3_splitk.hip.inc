// Deterministic split-K weight gradient of the 3x3/s1/p1 NHWC conv (gfx950),
// with the bias gradient fused: MOOLIB_AMD_WGRAD_KERNEL=2 (ops/conv3x3.py).
//
//   dW[k, c, kh, kw] = sum_{n,h,w} dy[n,k,h,w] * xpad[n,c,h+kh,w+kw]
//   db[k]            = sum_{n,h,w} dy[n,k,h,w]                       (optional)
//
// As a GEMM: P[kd, k] = sum_m A[m, kd] * dy[m, k] with kd = (kh*3+kw)*C + c and
// A the tap-shifted x; row 9C of P is db (A = 1). Both operands have the
// reduction axis (pixels) as their slow axis in memory, so both go through LDS
// transposed, the way lstm_input's wgrad does it, and an MFMA fragment
// (mfma_f32_16x16x32_bf16: A[lane&15][(lane>>4)*8+e], B[(lane>>4)*8+e][lane&15],
// D col = lane&15, row = (lane>>4)*4+reg) is 8 consecutive pixels of one channel.
//
// Work split. The N*ceil(H/R) slabs of R output rows of one image are dealt
// round-robin to G = min(slabs, kMaxGroups) workgroups of 4 waves. R and G are
// functions of (C, K, W) and of the shape (plan(), no environment override), so
// the order of every sum is fixed per shape. A workgroup keeps the whole
// [9C (+1), K] tile set in registers over all its slabs: wave w owns the
// 16-row kd tiles w, w+4, ... (at most 5) for every 16-column k tile, with
// compile-time accumulator indices (runtime ones would send acc to scratch).
//
// Staging. Per slab the x rows oh0-1 .. oh0+R and the dy rows oh0 .. oh0+R-1
// are read once, 16 bytes (8 channels) for each of two neighbouring pixels per
// lane, and written as 8 packed dwords to xT[row][c][pixel] / dT[row][k][pixel].
// A lane's item is (pixel pair = 32 consecutive per half wave, channel octet =
// half wave), and the row pitch in dwords is 4 * odd (PX = WP + 24, PD = WP + 8
// elements, WP = W rounded up to the 32-pixel chunk): the 64 dword writes of a
// wave go to banks pair + 32 * octet, and the 16-byte reads of a fragment, 16
// rows apart by the pitch, cover all 64 banks once. x pixel iw lies at column
// iw + 8. Zeroed: once per launch the columns no slab writes (left halo, right
// halo and the tail up to the chunk, in both buffers), and per slab the rows
// above/below the image, which the staging writes as zeros; never the slab.
// The x slab serves all nine taps. Tap kw = 1 is the aligned 16-byte read at
// column p0 + 8; kw = 0 / 2 add the aligned dword before / after it and form
// the fragment with four v_alignbyte (a 2-byte funnel shift) in registers.
//
// Overlap. Two LDS buffers; the global loads of the workgroup's next slab are
// issued before the MFMAs of this one and written to the other buffer after
// them; one barrier per slab. plan() keeps both buffers within kLdsMax = 64 KB,
// so two workgroups share a CU's 160 KB.
//
// Bias. The dy column sums are one more A row: row kd = 9C is all ones (bf16
// 1.0 times bf16 dy, fp32 accumulation: exact products). For C = 8 it sits in
// the zero padding of the fifth kd tile (72..79) and costs nothing; for C = 16
// and 32 it adds one kd tile.
//
// Reduce. Each workgroup stores its fp32 partial to ws[G][9C (+1)][K]; the
// second launch sums the G partials as four index-ordered quarters combined in
// a fixed order, drops channels c >= c_real and writes dW in nn.Conv2d's
// [K, c_real, 3, 3] order and db. No atomics: two runs agree bit for bit.
//
// Resource usage (-Rpass-analysis=kernel-resource-usage, gfx950): scratch 0
// everywhere; VGPRs + AGPRs and waves/SIMD of partial_kernel<C, K, db>:
//   C= 8 K=16: 146+4  (db 147+4),  3      C= 8 K=32: 138+16 (db 139+16), 3
//   C=16 K=16: 139+4  (db 141+4),  3      C=16 K=32: 140+24 (db 141+24), 3
//   C=32 K=16: 199+4  (db 201+4),  2      C=32 K=32: 141+40 (db 143+40), 2
// LDS is dynamic, both buffers, set by plan(): at the learner's shapes 49664 B
// (C=8 K=16 W=84, R=4), 52224 B (16/16, W=42, R=4), 55808 B (16/32, W=42, R=3),
// 63488 B (32/32, W=21 and 11, R=4); never above 65536 B. reduce_kernel: 43
// VGPRs, 1024 B of LDS.

namespace wgrad_splitk {

using bf16 = __bf16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using floatx4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;

constexpr int kThreads = 256;
constexpr int kMaxItems = 4;        // staged (pixel pair, channel octet) items per thread, x and dy each
constexpr int kMaxGroups = 512;     // workgroups, i.e. partials the reduce launch sums
constexpr int kLdsMax = 64 * 1024;  // both buffers; two workgroups per CU
constexpr int kRedParts = 4;        // index-ordered quarters of the reduce launch

// ---- host: the slab height R for (C, K, W), and the LDS it needs
struct Plan {
  int R = 0;        // output rows per slab; 0: no slab fits
  int WP = 0;       // W rounded up to whole 32-pixel chunks
  int PX = 0;       // x row pitch in elements
  int PD = 0;       // dy row pitch in elements
  size_t lds = 0;   // bytes, both buffers
};

inline int itemsFor(int rows, int W, int CH) {
  const int pairs = rows * ((W + 1) / 2);
  return (pairs + 31) / 32 * 32 * (CH / 8);
}

inline Plan plan(int C, int K, int W) {
  Plan p;
  p.WP = (W + 31) / 32 * 32;
  p.PX = p.WP + 24;
  p.PD = p.WP + 8;
  for (int R : {8, 6, 4, 3, 2, 1}) {
    const size_t lds =
        2 * sizeof(uint16_t) * ((size_t)(R + 2) * C * p.PX + (size_t)R * K * p.PD);
    if (lds <= (size_t)kLdsMax && itemsFor(R + 2, W, C) <= kMaxItems * kThreads &&
        itemsFor(R, W, K) <= kMaxItems * kThreads) {
      p.R = R;
      p.lds = lds;
      break;
    }
  }
  return p;
}

// ---- device
// One operand's slab on its way to LDS: this thread's items are the same in
// every slab, so their offsets are decoded once.
template <int CH>
struct Stager {
  int gofs[kMaxItems];  // element offset from the slab's first staged row; -1: no item
  int lofs[kMaxItems];  // element offset in the LDS buffer
  int row[kMaxItems];
  bool two[kMaxItems];  // the pair's second pixel is inside the row
  u32x4 v0[kMaxItems], v1[kMaxItems];

  DEV_INLINE void init(int tid, int rows, int W, int pitch, int col0) {
    constexpr int C8 = CH / 8;
    const int PP = (W + 1) / 2;
#pragma unroll
    for (int j = 0; j < kMaxItems; ++j) {
      const int idx = tid + j * kThreads;
      const int grp = idx >> 5;
      const int c8 = grp % C8;
      const int q = (grp / C8) * 32 + (idx & 31);
      const int r = q / PP, pp = q - r * PP;
      const bool ok = q < rows * PP;
      row[j] = r;
      two[j] = 2 * pp + 1 < W;
      gofs[j] = ok ? (r * W + 2 * pp) * CH + c8 * 8 : -1;
      lofs[j] = (r * CH + c8 * 8) * pitch + col0 + 2 * pp;
    }
  }

  // rows ih0 + row of the image at `img` ([H, W, CH]); rows outside it read as zero
  DEV_INLINE void fetch(const bf16* __restrict__ img, int ih0, int H, int W) {
    const bf16* base = img + (int64_t)ih0 * W * CH;
#pragma unroll
    for (int j = 0; j < kMaxItems; ++j) {
      v0[j] = v1[j] = u32x4{0u, 0u, 0u, 0u};
      const int ih = ih0 + row[j];
      if (gofs[j] >= 0 && ih >= 0 && ih < H) {
        v0[j] = *reinterpret_cast<const u32x4*>(base + gofs[j]);
        if (two[j]) v1[j] = *reinterpret_cast<const u32x4*>(base + gofs[j] + CH);
      }
    }
  }

  // channel c of pixels (2pp, 2pp+1) as one dword at [c][2pp]
  DEV_INLINE void store(bf16* buf, int pitch) const {
#pragma unroll
    for (int j = 0; j < kMaxItems; ++j) {
      if (gofs[j] < 0) continue;
      uint32_t* dst = reinterpret_cast<uint32_t*>(buf + lofs[j]);
      const int pd = pitch / 2;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        dst[(2 * i) * pd] = (v0[j][i] & 0xffffu) | (v1[j][i] << 16);
        dst[(2 * i + 1) * pd] = (v0[j][i] >> 16) | (v1[j][i] & 0xffff0000u);
      }
    }
  }
};

// A fragment of kd tile `tile` for output row r, pixels p0 .. p0+7: rows
// kd = tile*16 + (lane&15), x at slab row r + kh, columns p0 + kw - 1 + 8.
template <int C, bool DB>
DEV_INLINE bf16x8 loadA(const bf16* xT, int PX, int r, int p0, int tile, int lo) {
  // C >= 16: the tile lies in one tap (wave-uniform); C == 8: two taps per tile
  const int tap = C >= 16 ? (tile * 16) / C : tile * 2 + (lo >> 3);
  const int c = C >= 16 ? (tile * 16) % C + lo : (lo & 7);
  if (tap >= 9) {  // past the last tap: the ones row of db, then zero padding
    const bool ones = DB && (C >= 16 ? lo == 0 : lo == 8);
    const uint32_t w = ones ? 0x3f803f80u : 0u;  // bf16 1.0 twice
    return __builtin_bit_cast(bf16x8, (u32x4{w, w, w, w}));
  }
  const int kh = (tap * 11) >> 5, kw = tap - 3 * kh;
  const bf16* base = xT + ((r + kh) * C + c) * PX + p0 + 8;
  const u32x4 d = *reinterpret_cast<const u32x4*>(base);
  if (kw == 1) return __builtin_bit_cast(bf16x8, d);
  u32x4 f;
  if (kw == 0) {
    const uint32_t e = *reinterpret_cast<const uint32_t*>(base - 2);
    f[0] = __builtin_amdgcn_alignbyte(d[0], e, 2);
    f[1] = __builtin_amdgcn_alignbyte(d[1], d[0], 2);
    f[2] = __builtin_amdgcn_alignbyte(d[2], d[1], 2);
    f[3] = __builtin_amdgcn_alignbyte(d[3], d[2], 2);
  } else {
    const uint32_t e = *reinterpret_cast<const uint32_t*>(base + 8);
    f[0] = __builtin_amdgcn_alignbyte(d[1], d[0], 2);
    f[1] = __builtin_amdgcn_alignbyte(d[2], d[1], 2);
    f[2] = __builtin_amdgcn_alignbyte(d[3], d[2], 2);
    f[3] = __builtin_amdgcn_alignbyte(e, d[3], 2);
  }
  return __builtin_bit_cast(bf16x8, f);
}

template <int C, int K, bool DB>
__global__ __launch_bounds__(kThreads) void partial_kernel(
    const bf16* __restrict__ x,   // [N, H, W, C]
    const bf16* __restrict__ dy,  // [N, H, W, K]
    float* __restrict__ ws,       // [gridDim.x, 9C + DB, K]
    int NB, int H, int W, int R) {
  constexpr int ROWS = 9 * C + (DB ? 1 : 0);
  constexpr int KDT = (ROWS + 15) / 16;  // kd tiles: 5, 9 / 10, 18 / 19
  constexpr int NT = (KDT + 3) / 4;      // per wave
  constexpr int KT = K / 16;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lo = lane & 15, hi = lane >> 4;
  const int WP = (W + 31) & ~31, PX = WP + 24, PD = WP + 8;
  const int xElems = (R + 2) * C * PX, dElems = R * K * PD;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* xT = reinterpret_cast<bf16*>(smem);  // [2][R + 2][C][PX]
  bf16* dT = xT + 2 * xElems;                // [2][R][K][PD]

  // the columns no slab writes, both buffers: x [0, 8) and [8 + 2*ceil(W/2), PX),
  // dy [2*ceil(W/2), PD)
  {
    const int w2 = (W + 1) & ~1;
    uint32_t* xd = reinterpret_cast<uint32_t*>(xT);
    for (int row = tid; row < 2 * (R + 2) * C; row += kThreads) {
      uint32_t* p = xd + row * (PX / 2);
      for (int i = 0; i < 4; ++i) p[i] = 0u;
      for (int i = (8 + w2) / 2; i < PX / 2; ++i) p[i] = 0u;
    }
    uint32_t* dd = reinterpret_cast<uint32_t*>(dT);
    for (int row = tid; row < 2 * R * K; row += kThreads) {
      uint32_t* p = dd + row * (PD / 2);
      for (int i = w2 / 2; i < PD / 2; ++i) p[i] = 0u;
    }
  }

  Stager<C> sx;
  Stager<K> sd;
  sx.init(tid, R + 2, W, PX, 8);
  sd.init(tid, R, W, PD, 0);

  floatx4 acc[NT][KT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) acc[i][kt] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int slabsPerImage = (H + R - 1) / R;
  const int slabs = NB * slabsPerImage;
  auto fetch = [&](int s) {
    const int n = s / slabsPerImage, oh0 = (s - n * slabsPerImage) * R;
    sx.fetch(x + (int64_t)n * H * W * C, oh0 - 1, H, W);
    sd.fetch(dy + (int64_t)n * H * W * K, oh0, H, W);
  };
  auto stage = [&](int buf) {
    sx.store(xT + buf * xElems, PX);
    sd.store(dT + buf * dElems, PD);
  };

  int s = blockIdx.x;  // gridDim.x <= slabs
  fetch(s);
  stage(0);
  __syncthreads();
  for (int buf = 0; s < slabs; s += gridDim.x, buf ^= 1) {
    const bool more = s + (int)gridDim.x < slabs;
    if (more) fetch(s + gridDim.x);
    const int rows = min(R, H - (s % slabsPerImage) * R);
    const bf16* xb = xT + buf * xElems;
    const bf16* db_ = dT + buf * dElems;
    for (int r = 0; r < rows; ++r) {
      for (int p0 = hi * 8; p0 < WP; p0 += 32) {
        bf16x8 b[KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
          b[kt] = *reinterpret_cast<const bf16x8*>(db_ + (r * K + kt * 16 + lo) * PD + p0);
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          const int tile = wave + 4 * i;
          if (tile < KDT) {
            const bf16x8 a = loadA<C, DB>(xb, PX, r, p0, tile, lo);
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
              acc[i][kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[kt], acc[i][kt], 0, 0, 0);
          }
        }
      }
    }
    if (more) stage(buf ^ 1);
    // the only barrier of the slab: buffer buf^1 is complete before the next
    // slab reads it, and was last read before the previous barrier
    __syncthreads();
  }

  float* mine = ws + (int64_t)blockIdx.x * ROWS * K;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int tile = wave + 4 * i;
    if (tile < KDT) {
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int kd = tile * 16 + hi * 4 + reg;
          if (kd < ROWS) mine[kd * K + kt * 16 + lo] = acc[i][kt][reg];
        }
    }
  }
}

// ws [G, rows, K] -> dW [K, cReal, 3, 3] and db [K] (row 9C, when rows > 9C).
// Thread (element, quarter) sums its quarter of the partials in index order;
// the four quarters are then added in a fixed order.
__global__ __launch_bounds__(kThreads) void reduce_kernel(
    const float* __restrict__ ws, float* __restrict__ dW, float* __restrict__ db,
    int G, int rows, int C, int K, int cReal) {
  __shared__ float sRed[kRedParts][64];
  const int elems = rows * K;
  const int el = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + el;
  const int per = (G + kRedParts - 1) / kRedParts;
  const int pEnd = min(G, (part + 1) * per);
  float sum = 0.f;
  if (e < elems) {
#pragma unroll 8
    for (int p = part * per; p < pEnd; ++p) sum += ws[(int64_t)p * elems + e];
  }
  sRed[part][el] = sum;
  __syncthreads();
  if (part != 0 || e >= elems) return;
  const float t = ((sRed[0][el] + sRed[1][el]) + sRed[2][el]) + sRed[3][el];
  const int kd = e / K, k = e - kd * K;
  if (kd == 9 * C) {
    db[k] = t;
    return;
  }
  const int tap = kd / C, c = kd - tap * C;
  if (c < cReal) dW[(k * cReal + c) * 9 + tap] = t;
}

template <int C, int K, bool DB>
void launchPartial(int G, size_t lds, hipStream_t stream, const bf16* x, const bf16* dy,
                   float* ws, int NB, int H, int W, int R) {
  hipLaunchKernelGGL((partial_kernel<C, K, DB>), dim3(G), dim3(kThreads), lds, stream, x, dy, ws,
                     NB, H, W, R);
}

}  // namespace wgrad_splitk

// Rows per slab the kernel uses for (C, K, W); 0 when no slab fits.
int64_t wgrad3x3_splitk_rows(int64_t C, int64_t K, int64_t W) {
  return wgrad_splitk::plan((int)C, (int)K, (int)W).R;
}

// x [N,C,H,W], dy [N,K,H,W], both bf16 channels_last -> (dW fp32 [K, c_real, 3, 3],
// db fp32 [K] or an empty tensor). Channels c >= c_real of x are ignored.
std::tuple<at::Tensor, at::Tensor> wgrad3x3_splitk(at::Tensor x, at::Tensor dy, int64_t c_real,
                                                   bool want_db) {
  namespace sk = wgrad_splitk;
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.scalar_type() == at::kBFloat16,
              "wgrad3x3_splitk: bf16 4D CUDA x expected");
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 4 && dy.scalar_type() == at::kBFloat16,
              "wgrad3x3_splitk: bf16 4D CUDA dy expected");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast), "wgrad3x3_splitk: x channels_last");
  TORCH_CHECK(dy.is_contiguous(at::MemoryFormat::ChannelsLast),
              "wgrad3x3_splitk: dy channels_last");
  TORCH_CHECK(x.get_device() == dy.get_device(), "wgrad3x3_splitk: x and dy on one device");
  const int64_t NB = x.size(0), H = x.size(2), W = x.size(3);
  const int C = (int)x.size(1), K = (int)dy.size(1);
  TORCH_CHECK(C == 8 || C == 16 || C == 32, "wgrad3x3_splitk: C in {8,16,32}, got ", C);
  TORCH_CHECK(K == 16 || K == 32, "wgrad3x3_splitk: K in {16,32}, got ", K);
  TORCH_CHECK(c_real >= 1 && c_real <= C, "wgrad3x3_splitk: c_real in [1, C], got ", c_real);
  TORCH_CHECK(dy.size(0) == NB && dy.size(2) == H && dy.size(3) == W,
              "wgrad3x3_splitk: x and dy differ in N, H or W");
  TORCH_CHECK(NB > 0 && H > 0 && W > 0, "wgrad3x3_splitk: empty input");
  TORCH_CHECK(NB * H * W * std::max(C, K) < (int64_t)INT_MAX,
              "wgrad3x3_splitk: input too large for 32-bit slab counts");
  const sk::Plan p = sk::plan(C, K, (int)W);
  TORCH_CHECK(p.R > 0, "wgrad3x3_splitk: W=", W, " too wide for C=", C, ", K=", K,
              " (a one-row slab does not fit the ", sk::kLdsMax / 1024, " KB of LDS)");
  const int slabs = (int)(NB * ((H + p.R - 1) / p.R));
  const int G = std::min(slabs, sk::kMaxGroups);
  const int rows = 9 * C + (want_db ? 1 : 0);
  const auto f32 = x.options().dtype(at::kFloat);
  auto ws = at::empty({G, rows, K}, f32);
  auto dw = at::empty({K, c_real, 3, 3}, f32);
  auto db = at::empty({want_db ? K : 0}, f32);
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  const sk::bf16* xp = reinterpret_cast<const sk::bf16*>(x.data_ptr());
  const sk::bf16* dyp = reinterpret_cast<const sk::bf16*>(dy.data_ptr());
  float* wsp = ws.data_ptr<float>();
#define WGRAD_SPLITK_CASE(CC, KK)                                                            \
  if (C == CC && K == KK) {                                                                  \
    if (want_db)                                                                             \
      sk::launchPartial<CC, KK, true>(G, p.lds, stream, xp, dyp, wsp, (int)NB, (int)H, (int)W, p.R); \
    else                                                                                     \
      sk::launchPartial<CC, KK, false>(G, p.lds, stream, xp, dyp, wsp, (int)NB, (int)H, (int)W, p.R); \
  }
  WGRAD_SPLITK_CASE(8, 16)
  WGRAD_SPLITK_CASE(8, 32)
  WGRAD_SPLITK_CASE(16, 16)
  WGRAD_SPLITK_CASE(16, 32)
  WGRAD_SPLITK_CASE(32, 16)
  WGRAD_SPLITK_CASE(32, 32)
#undef WGRAD_SPLITK_CASE
  hipLaunchKernelGGL(sk::reduce_kernel, dim3((rows * K + 63) / 64), dim3(sk::kThreads), 0, stream,
                     wsp, dw.data_ptr<float>(), want_db ? db.data_ptr<float>() : nullptr, G, rows,
                     C, K, (int)c_real);
  return {dw, db};
}
