// Weight-gradient (wrw) for the 3x3/s1/p1 NHWC conv on MFMA (gfx950).
//
// dW[kd, n] = sum_m A[m, kd] * dy[m, n] with kd = (kh*3+kw)*C + c and
// A[m, kd] = x at pixel m shifted by the tap (zero-padded) — a tall-skinny
// GEMM reduced over every output pixel. The kernel processes a SLAB of R
// consecutive output rows of one image per staging phase: x rows
// oh0-1..oh0+R are staged TRANSPOSED to LDS ([(R+2)][C][W+2+pad], halo and
// tail columns zeroed) so an A fragment (one kd, 8 adjacent pixels in a
// row) is 8 contiguous bf16, and dy's R rows are staged transposed the
// same way ([R][K][Wpad]). One __syncthreads pair then covers
// R*ceil(W/32) MFMA reduction chunks (the r1 version staged one row per
// sync and was sync/latency-bound, 3-5x slower than MIOpen). Each wave
// owns a kd-tile range and atomically folds its fp32 tile into the global
// [9C-padded, K] output once at the end.
//
// Reordering [9C, K] -> [K, C, 3, 3] is a trivial torch permute on 9K*C
// elements (ops/conv3x3.py).

namespace wgrad3x3 {

using bf16 = __bf16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using floatx4 = __attribute__((ext_vector_type(4))) float;

constexpr int kMaxKdTilesPerWave = 5;  // ceil(18 kd-tiles / 4 waves) for C=32

template <int C>
__global__ __launch_bounds__(256) void wgrad3x3_nhwc_kernel(
    const bf16* __restrict__ x,   // [N, H, W, C]
    const bf16* __restrict__ dy,  // [N, H, W, K]
    float* __restrict__ out,      // [kdTiles16 * 16, K] zero-initialized
    int NB, int H, int W, int K, int R) {
  constexpr int KD = 9 * C;
  constexpr int KDT = (KD + 15) / 16;  // kd tiles (C=16 -> 9, C=32 -> 18)
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int lo = lane & 15, hi = lane >> 4;
  const int nCt = K >> 4;
  const int WP = (W + 31) & ~31;   // reduction-padded row length
  const int COLS = WP + 2;         // staged x columns: iw -1 .. WP (zero edges)

  extern __shared__ char smem[];
  bf16* xT = reinterpret_cast<bf16*>(smem);             // [(R+2)][C][COLS]
  bf16* dyT = xT + (R + 2) * C * COLS;                  // [R][K][WP]

  // Wave's kd tiles: wave w owns tiles w, w+4, w+8, ...  All loops over
  // (tile, ct) are FULLY UNROLLED with compile-time indices — dynamic
  // indexing of acc[][] sends the accumulators to scratch memory (176
  // B/lane measured) and every MFMA becomes a global-memory RMW.
  constexpr int NT = (KDT + 3) / 4;  // tiles per wave upper bound
  floatx4 acc[NT][2];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) acc[i][ct] = (floatx4){0.f, 0.f, 0.f, 0.f};

  const int batchesPerImage = (H + R - 1) / R;
  const int totalBatches = NB * batchesPerImage;
  constexpr int C8 = C / 8;
  const int K8 = K / 8;
  const int ldsElems = (R + 2) * C * COLS + R * K * WP;

  for (int batch = blockIdx.x; batch < totalBatches; batch += gridDim.x) {
    const int n = batch / batchesPerImage;
    const int oh0 = (batch % batchesPerImage) * R;
    __syncthreads();  // previous slab's reads done before restage
    // ---- zero both slabs (vectorized; ldsElems is a multiple of 8) ----
    {
      bf16x8 z;
#pragma unroll
      for (int e = 0; e < 8; ++e) z[e] = (bf16)0.f;
      for (int idx = threadIdx.x; idx < ldsElems / 8; idx += blockDim.x) {
        *reinterpret_cast<bf16x8*>(xT + idx * 8) = z;
      }
      for (int t = ldsElems / 8 * 8 + threadIdx.x; t < ldsElems; t += blockDim.x) {
        xT[t] = (bf16)0.f;
      }
    }
    __syncthreads();
    // ---- stage x rows oh0-1 .. oh0+R: one coalesced bf16x8 load per
    // (slabRow, iw, c-octet), scattered to the transposed slab; for C=4
    // (the first conv) each 8-element load covers TWO pixels ----
    if constexpr (C >= 8) {
      for (int idx = threadIdx.x; idx < (R + 2) * C8 * W; idx += blockDim.x) {
        int iw = idx % W;
        int rest = idx / W;
        int c8 = rest % C8;
        int sr = rest / C8;  // slab row: x row oh0 + sr - 1
        int ih = oh0 + sr - 1;
        if (ih < 0 || ih >= H) continue;
        bf16x8 v = *reinterpret_cast<const bf16x8*>(
            x + (((int64_t)n * H + ih) * W + iw) * C + c8 * 8);
        const int col = iw + 1;
#pragma unroll
        for (int e = 0; e < 8; ++e) xT[((int64_t)sr * C + c8 * 8 + e) * COLS + col] = v[e];
      }
    } else {
      const int wPairs = (W + 1) / 2;
      for (int idx = threadIdx.x; idx < (R + 2) * wPairs; idx += blockDim.x) {
        int p = idx % wPairs;
        int sr = idx / wPairs;
        int ih = oh0 + sr - 1;
        if (ih < 0 || ih >= H) continue;
        int iw = p * 2;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          if (iw + q >= W) break;
          const bf16* src = x + (((int64_t)n * H + ih) * W + iw + q) * C;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            xT[((int64_t)sr * C + c) * COLS + iw + q + 1] = src[c];
          }
        }
      }
    }
    // ---- stage dy rows oh0 .. oh0+R-1 the same way ----
    for (int idx = threadIdx.x; idx < R * K8 * W; idx += blockDim.x) {
      int ow = idx % W;
      int rest = idx / W;
      int k8 = rest % K8;
      int r = rest / K8;
      int oh = oh0 + r;
      if (oh >= H) continue;  // stays zero -> contributes nothing
      bf16x8 v = *reinterpret_cast<const bf16x8*>(
          dy + (((int64_t)n * H + oh) * W + ow) * K + k8 * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) dyT[((int64_t)r * K + k8 * 8 + e) * WP + ow] = v[e];
    }
    __syncthreads();

    // ---- MFMA over the slab's R * WP pixels ----
    for (int r = 0; r < R; ++r) {
      for (int chunk = 0; chunk < WP / 32; ++chunk) {
        const int pix0 = chunk * 32 + hi * 8;  // this lane's 8 reduction pixels
        bf16x8 b[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          if (ct < nCt) {
            b[ct] = *reinterpret_cast<const bf16x8*>(
                dyT + ((int64_t)r * K + ct * 16 + lo) * WP + pix0);
          }
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          const int tile = wave + 4 * i;
          if (tile >= KDT) break;
          const int kd = tile * 16 + lo;
          bf16x8 a;
          if (kd < KD) {
            const int tap = kd / C;
            const int c = kd % C;
            const int dh = tap / 3, dw = tap % 3;
            // A fragment: slab row r+dh, staged column pix0+dw, 8
            // contiguous bf16 (2-byte aligned -> memcpy lets the
            // compiler emit legal LDS reads)
            const bf16* src = xT + ((int64_t)(r + dh) * C + c) * COLS + pix0 + dw;
            __builtin_memcpy(&a, src, sizeof(a));
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] = (bf16)0.f;
          }
#pragma unroll
          for (int ct = 0; ct < 2; ++ct) {
            if (ct < nCt) {
              acc[i][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[ct], acc[i][ct], 0, 0, 0);
            }
          }
        }
      }
    }
  }

  // ---- write this workgroup's partial: out[blockIdx][kd][n] (plain
  // stores — atomics to the tiny shared [9C,K] from 512-1024 WGs formed
  // per-address RMW chains; a second kernel folds the partials) ----
  float* mine = out + (int64_t)blockIdx.x * (KDT * 16) * K;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int tile = wave + 4 * i;
    if (tile >= KDT) break;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      if (ct >= nCt) break;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int kd = tile * 16 + hi * 4 + reg;
        mine[(int64_t)kd * K + ct * 16 + lo] = acc[i][ct][reg];
      }
    }
  }
}

// Fold partials[p][e] -> out[e]. Parallel over (elem, partial-chunk): with
// only ~1.5-9k output elems, a one-thread-per-elem loop over 512+ partials
// was the whole kernel's runtime; 16 chunk-threads per elem read
// coalesced rows and combine with a short atomic chain.
constexpr int kFoldChunks = 16;

__global__ void wgrad3x3_fold_kernel(const float* __restrict__ partials,
                                     float* __restrict__ out, int nPartials, int elems) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= elems * kFoldChunks) return;
  int e = t % elems;
  int chunk = t / elems;
  int per = (nPartials + kFoldChunks - 1) / kFoldChunks;
  int p0 = chunk * per;
  int p1 = min(p0 + per, nPartials);
  float s = 0.f;
  for (int p = p0; p < p1; ++p) s += partials[(int64_t)p * elems + e];
  atomicAdd(&out[e], s);  // out is zero-initialized; depth <= kFoldChunks
}

}  // namespace wgrad3x3

// dW for conv3x3/s1/p1: x [N,C,H,W] channels_last bf16, dy [N,K,H,W]
// channels_last bf16 -> fp32 [KDT*16, K] GEMM-layout gradient (caller
// reorders to [K, C, 3, 3]).
at::Tensor wgrad3x3_nhwc(at::Tensor x, at::Tensor dy) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.scalar_type() == at::kBFloat16,
              "wgrad3x3: bf16 4D CUDA x expected");
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 4 && dy.scalar_type() == at::kBFloat16,
              "wgrad3x3: bf16 4D CUDA dy expected");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast), "wgrad3x3: x channels_last");
  TORCH_CHECK(dy.is_contiguous(at::MemoryFormat::ChannelsLast), "wgrad3x3: dy channels_last");
  const int NB = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int K = dy.size(1);
  TORCH_CHECK(C == 4 || C == 8 || C == 16 || C == 32, "wgrad3x3: C in {4,8,16,32}");
  TORCH_CHECK(K == 16 || K == 32, "wgrad3x3: K in {16,32}");
  TORCH_CHECK(dy.size(0) == NB && dy.size(2) == H && dy.size(3) == W, "wgrad3x3: shape mismatch");
  const int KDT = (9 * C + 15) / 16;
  auto out = at::zeros({KDT * 16, K}, x.options().dtype(at::kFloat));
  const int WP = (W + 31) & ~31;
  // Largest row-slab R whose LDS fits ~48 KB (leaves room for 2+ workgroups
  // per CU against the 160 KB CDNA4 LDS).
  int R = 0;
  size_t lds = 0;
  for (int cand : {8, 6, 4, 3, 2, 1}) {
    size_t need = sizeof(uint16_t) * ((size_t)(cand + 2) * C * (WP + 2) + (size_t)cand * K * WP);
    if (need <= 48 * 1024) {
      R = cand;
      lds = need;
      break;
    }
  }
  // the kernel stages full-width rows: with no slab there is no LDS to run in
  TORCH_CHECK(R > 0, "wgrad3x3: W=", W, " too wide for C=", C, ", K=", K,
              " (a one-row slab needs more than 48 KB of LDS)");
  TORCH_CHECK(NB > 0 && H > 0 && W > 0, "wgrad3x3: empty input");
  const int totalBatches = NB * ((H + R - 1) / R);
  // ~totalBatches/4 capped at 1024 measured best (profiles/evidence/r2l_sweep.txt);
  // fewer blocks also shrink the partial buffer the fold pass reads.
  int maxBlocks = std::min(std::max(totalBatches / 4, 64), 1024);
  if (const char* e = std::getenv("MOOLIB_AMD_WGRAD_BLOCKS")) maxBlocks = std::atoi(e);
  const int blocks = std::max(1, std::min(totalBatches, maxBlocks));
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  using wgrad3x3::bf16;
  const bf16* xp = reinterpret_cast<const bf16*>(x.data_ptr());
  const bf16* dyp = reinterpret_cast<const bf16*>(dy.data_ptr());
  const int elems = KDT * 16 * K;
  auto partials = at::empty({blocks, KDT * 16, K}, x.options().dtype(at::kFloat));
  float* pp = partials.data_ptr<float>();
  if (C == 4) {
    hipLaunchKernelGGL((wgrad3x3::wgrad3x3_nhwc_kernel<4>), dim3(blocks), dim3(256), lds,
                       stream, xp, dyp, pp, NB, H, W, K, R);
  } else if (C == 8) {
    hipLaunchKernelGGL((wgrad3x3::wgrad3x3_nhwc_kernel<8>), dim3(blocks), dim3(256), lds,
                       stream, xp, dyp, pp, NB, H, W, K, R);
  } else if (C == 16) {
    hipLaunchKernelGGL((wgrad3x3::wgrad3x3_nhwc_kernel<16>), dim3(blocks), dim3(256), lds,
                       stream, xp, dyp, pp, NB, H, W, K, R);
  } else {
    hipLaunchKernelGGL((wgrad3x3::wgrad3x3_nhwc_kernel<32>), dim3(blocks), dim3(256), lds,
                       stream, xp, dyp, pp, NB, H, W, K, R);
  }
  hipLaunchKernelGGL(wgrad3x3::wgrad3x3_fold_kernel,
                     dim3((elems * wgrad3x3::kFoldChunks + 255) / 256), dim3(256), 0,
                     stream, pp, out.data_ptr<float>(), blocks, elems);
  return out;
}
