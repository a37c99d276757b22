// Fused 3x3/s1/p1 NHWC conv on MFMA for the actor inference path (gfx950).
//
// The IMPALA residual block is conv(relu(x)) -> conv(relu(.)) -> +x
// (reference examples/atari/models.py:30-42). MIOpen runs each conv as a
// standalone igemm plus separate bias/relu/add passes; this kernel computes
// the conv as an implicit GEMM on v_mfma_f32_16x16x32_bf16 with
//   - the producer relu (+ optional pending per-channel bias) applied ON
//     LOAD of the input fragment, and
//   - bias / bias+relu / bias+residual(+bias2) applied ON STORE,
// so one residual block is TWO kernel launches and the activation tensor
// crosses HBM once per conv. Forward-only (actor runs under no_grad; the
// learner keeps MIOpen + autograd).
//
// GEMM view: M = N*H*W output pixels, Ndim = K out-channels, Kdim = 9*C.
// Fragment conventions identical to lstm.hip.inc / ops/lstm.py pack_mfma_b:
//   A[i][k]: i = lane&15 (pixel), k = (lane>>4)*8 + e  (one bf16x8 load)
//   B packed so fragment (ct,kk) lane l reads 8 contiguous bf16
//   D[r][c]: c = ct*16 + (lane&15), r = (lane>>4)*4 + reg
// Each wave owns a 16-pixel M-tile and loops ct over K/16 N-tiles and kk
// over ceil(9C/32) K-chunks. A-lane's 8 elements never straddle a filter
// tap because C % 8 == 0 and taps are C-aligned in Kdim.

namespace conv3x3 {

using bf16 = __bf16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using floatx4 = __attribute__((ext_vector_type(4))) float;

#define C3_DEV static __device__ __forceinline__

C3_DEV bf16x8 zero8() {
  bf16x8 z;
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = (bf16)0.f;
  return z;
}

// epilogue codes
enum { kEpiNone = 0, kEpiBias = 1, kEpiBiasRelu = 2, kEpiBiasAdd = 3 };

// RT = row-tiles per wave (v2): each wave owns RT consecutive 16-pixel
// M-tiles, giving RT independent MFMA accumulation chains (hides the MFMA
// result latency that a single serial D-chain stalls on) AND reusing each
// B fragment across RT tiles (RTx fewer B loads). RT is chosen by M on the
// host: big layers use RT=4, small ones keep RT=1 so the launch still
// fills 256 CUs.
template <int C, bool RELU_IN, int RT>
__global__ __launch_bounds__(256) void conv3x3_nhwc_kernel(
    const bf16* __restrict__ x,        // [N, H, W, C] (channels_last)
    const bf16* __restrict__ wPacked,  // packed B fragments, Kdim KK*32 x K
    const bf16* __restrict__ biasIn,   // [C] pending bias on the input, or null
    bf16* __restrict__ out,            // [N, H, W, K]
    const bf16* __restrict__ bias1,    // [K] epilogue bias, or null
    const bf16* __restrict__ res,      // [N, H, W, K] residual, or null
    const bf16* __restrict__ bias2,    // [K] second epilogue bias, or null
    int NB, int H, int W, int K, int epi) {
  constexpr int KK = (9 * C + 31) / 32;  // K-chunks
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int lo = lane & 15, hi = lane >> 4;
  const int64_t M = (int64_t)NB * H * W;
  const int64_t pixBase = ((int64_t)blockIdx.x * 4 + wave) * (16 * RT);
  if (pixBase >= M) return;

  // Decode each row-tile's A-row pixel once (same for every chunk).
  int an[RT], aoh[RT], aow[RT];
  bool aok[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int64_t apix = pixBase + rt * 16 + lo;
    aok[rt] = apix < M;
    an[rt] = aoh[rt] = aow[rt] = 0;
    if (aok[rt]) {
      int64_t r = apix;
      aow[rt] = (int)(r % W);
      r /= W;
      aoh[rt] = (int)(r % H);
      an[rt] = (int)(r / H);
    }
  }
  const int nCt = K >> 4;
  // RT==1 keeps v1's even/odd-kk chain split (two independent chains);
  // RT>=2 gets its chains from the row tiles themselves.
  constexpr int CH = (RT == 1) ? 2 : RT;
  floatx4 acc[CH][2];  // [chain][ct], K <= 32 in this model family
#pragma unroll
  for (int ch = 0; ch < CH; ++ch)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) acc[ch][ct] = (floatx4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    // ---- A fragments: 8 input elems of one tap for each row-tile ----
    const int kd = kk * 32 + hi * 8;
    const int tap = kd / C;
    const int c0 = kd % C;
    bf16x8 a[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      a[rt] = zero8();
      if (aok[rt] && tap < 9) {
        const int ih = aoh[rt] + tap / 3 - 1;
        const int iw = aow[rt] + tap % 3 - 1;
        if (ih >= 0 && ih < H && iw >= 0 && iw < W) {
          const bf16* p = x + ((((int64_t)an[rt] * H + ih) * W + iw) * C + c0);
          a[rt] = *reinterpret_cast<const bf16x8*>(p);
          if (RELU_IN) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              float v = (float)a[rt][e];
              if (biasIn != nullptr) v += (float)biasIn[c0 + e];
              a[rt][e] = (bf16)(v > 0.f ? v : 0.f);
            }
          }
        }
        // padding pixel: pad(relu(x+b)) pads with zeros — zero8 is correct.
      }
    }
    // ---- B fragments + MFMA per N-tile, B reused across row-tiles ----
    for (int ct = 0; ct < nCt; ++ct) {
      const bf16* bp = wPacked + (((int64_t)ct * KK + kk) * 64 + lane) * 8;
      bf16x8 b = *reinterpret_cast<const bf16x8*>(bp);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const int ch = (RT == 1) ? (kk & 1) : rt;
        acc[ch][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[rt], b, acc[ch][ct], 0, 0, 0);
      }
    }
  }

  // ---- epilogue + store: rows hi*4+reg, col ct*16+lo ----
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    for (int ct = 0; ct < nCt; ++ct) {
      const int col = ct * 16 + lo;
      const float b1 = (bias1 != nullptr) ? (float)bias1[col] : 0.f;
      const float b2 = (bias2 != nullptr) ? (float)bias2[col] : 0.f;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t pix = pixBase + rt * 16 + hi * 4 + reg;
        if (pix >= M) continue;
        float v = (RT == 1) ? (acc[0][ct][reg] + acc[1][ct][reg]) : acc[rt][ct][reg];
        if (epi == kEpiBias) {
          v += b1;
        } else if (epi == kEpiBiasRelu) {
          v += b1;
          v = v > 0.f ? v : 0.f;
        } else if (epi == kEpiBiasAdd) {
          v += b1 + b2 + (float)res[pix * K + col];
        }
        out[pix * K + col] = (bf16)v;
      }
    }
  }
}

// LDS band-slab variant: a workgroup owns a band of BR image rows (full
// width). The (BR+2) x (W+2) x C input slab is staged to LDS ONCE — with
// the producer relu(+bias) applied at staging — and every tap read comes
// from LDS, so the activation crosses global memory once instead of ~9
// gather reads per pixel (v1 is gather-latency bound at the small-W
// layers). Fragment maps, kk-parity chains and the store epilogue are
// identical to the flat kernel above.
template <int C, bool RELU_IN>
__global__ __launch_bounds__(256) void conv3x3_nhwc_lds_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ wPacked,
    const bf16* __restrict__ biasIn, bf16* __restrict__ out,
    const bf16* __restrict__ bias1, const bf16* __restrict__ res,
    const bf16* __restrict__ bias2, int NB, int H, int W, int K, int epi, int BR) {
  constexpr int KK = (9 * C + 31) / 32;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int lo = lane & 15, hi = lane >> 4;
  const int nCt = K >> 4;
  const int WS = W + 2;  // slab columns (iw -1..W)

  extern __shared__ char smem[];
  bf16* slab = reinterpret_cast<bf16*>(smem);  // [(BR+2)][WS][C]

  const int bandsPerImage = (H + BR - 1) / BR;
  const int band = blockIdx.x % bandsPerImage;
  const int n = blockIdx.x / bandsPerImage;
  const int row0 = band * BR;
  const int bandRows = min(BR, H - row0);
  const int bandPix = bandRows * W;

  // ---- stage the slab: rows row0-1 .. row0+bandRows, zero-edged, with
  // the producer relu(+bias) fused in ----
  constexpr int C8 = C / 8;
  {
    // zero left/right halo columns + OOB rows are handled by staging the
    // full slab with bounds checks (slab is small; one pass).
    for (int idx = threadIdx.x; idx < (BR + 2) * WS * C8; idx += blockDim.x) {
      int c8 = idx % C8;
      int rest = idx / C8;
      int col = rest % WS;
      int sr = rest / WS;
      if (sr >= bandRows + 2) break;
      const int ih = row0 + sr - 1;
      const int iw = col - 1;
      bf16x8 v = zero8();
      if (ih >= 0 && ih < H && iw >= 0 && iw < W) {
        v = *reinterpret_cast<const bf16x8*>(
            x + ((((int64_t)n * H + ih) * W + iw) * C + c8 * 8));
        if (RELU_IN) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float f = (float)v[e];
            if (biasIn != nullptr) f += (float)biasIn[c8 * 8 + e];
            v[e] = (bf16)(f > 0.f ? f : 0.f);
          }
        }
      }
      *reinterpret_cast<bf16x8*>(slab + ((int64_t)sr * WS + col) * C + c8 * 8) = v;
    }
  }
  __syncthreads();

  // ---- flat 16-pixel M-tiles over the band, waves round-robin ----
  const int nTiles = (bandPix + 15) / 16;
  for (int tile = wave; tile < nTiles; tile += 4) {
    const int p = tile * 16 + lo;  // pixel within the band (this lane's A row)
    const bool aok = p < bandPix;
    const int pr = aok ? p / W : 0;   // band-relative row
    const int pc = aok ? p % W : 0;
    floatx4 acc[2][2];
#pragma unroll
    for (int pq = 0; pq < 2; ++pq)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) acc[pq][ct] = (floatx4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      const int kd = kk * 32 + hi * 8;
      const int tap = kd / C;
      const int c0 = kd % C;
      bf16x8 a = zero8();
      if (aok && tap < 9) {
        // slab holds zero-padded, relu'ed input: no bounds math here
        const int sr = pr + tap / 3;        // +dh with the -1 halo baked in
        const int sc = pc + tap % 3;
        a = *reinterpret_cast<const bf16x8*>(slab + ((int64_t)sr * WS + sc) * C + c0);
      }
      for (int ct = 0; ct < nCt; ++ct) {
        const bf16* bp = wPacked + (((int64_t)ct * KK + kk) * 64 + lane) * 8;
        bf16x8 b = *reinterpret_cast<const bf16x8*>(bp);
        acc[kk & 1][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[kk & 1][ct], 0, 0, 0);
      }
    }
    // ---- epilogue + store (identical to the flat kernel) ----
    const int64_t imgBase = ((int64_t)n * H + row0) * W;
    for (int ct = 0; ct < nCt; ++ct) {
      const int col = ct * 16 + lo;
      const float b1 = (bias1 != nullptr) ? (float)bias1[col] : 0.f;
      const float b2 = (bias2 != nullptr) ? (float)bias2[col] : 0.f;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int pp = tile * 16 + hi * 4 + reg;
        if (pp >= bandPix) continue;
        const int64_t pix = imgBase + pp;
        float v = acc[0][ct][reg] + acc[1][ct][reg];
        if (epi == kEpiBias) {
          v += b1;
        } else if (epi == kEpiBiasRelu) {
          v += b1;
          v = v > 0.f ? v : 0.f;
        } else if (epi == kEpiBiasAdd) {
          v += b1 + b2 + (float)res[pix * K + col];
        }
        out[pix * K + col] = (bf16)v;
      }
    }
  }
}

}  // namespace conv3x3

at::Tensor conv3x3_nhwc_fused(at::Tensor x, at::Tensor wPacked, int64_t K,
                              bool reluIn, c10::optional<at::Tensor> biasIn,
                              int64_t epi, c10::optional<at::Tensor> bias1,
                              c10::optional<at::Tensor> res,
                              c10::optional<at::Tensor> bias2,
                              int64_t rtOverride) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.scalar_type() == at::kBFloat16,
              "conv3x3: bf16 4D CUDA tensor expected");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast), "conv3x3: channels_last expected");
  const int NB = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(C == 8 || C == 16 || C == 32, "conv3x3: C in {8,16,32}");
  TORCH_CHECK(K == 16 || K == 32, "conv3x3: K in {16,32}");
  TORCH_CHECK(epi >= conv3x3::kEpiNone && epi <= conv3x3::kEpiBiasAdd, "conv3x3: epi in 0..3");
  TORCH_CHECK(rtOverride <= 0 || rtOverride == 1 || rtOverride == 2 || rtOverride == 4,
              "conv3x3: rt in {1,2,4}");
  // The kernel indexes every operand from C, K and the output shape alone:
  // reject anything it would read out of range or reinterpret.
  auto checkVec = [&](const at::Tensor& t, int64_t n, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == x.device() && t.scalar_type() == at::kBFloat16 &&
                    t.is_contiguous(),
                "conv3x3: ", name, " must be a contiguous bf16 tensor on x's device");
    TORCH_CHECK(t.numel() == n, "conv3x3: ", name, " has ", t.numel(), " elements, expected ", n);
  };
  checkVec(wPacked, (int64_t)((9 * C + 31) / 32) * 32 * K, "w_packed");
  if (biasIn.has_value()) checkVec(*biasIn, C, "bias_in");
  TORCH_CHECK(epi == conv3x3::kEpiNone || bias1.has_value(), "conv3x3: epi ", epi,
              " needs bias1");
  if (bias1.has_value()) checkVec(*bias1, K, "bias1");
  if (bias2.has_value()) checkVec(*bias2, K, "bias2");
  TORCH_CHECK(epi != conv3x3::kEpiBiasAdd || res.has_value(), "conv3x3: epi 3 needs res");
  if (res.has_value()) {
    TORCH_CHECK(res->is_cuda() && res->device() == x.device() &&
                    res->scalar_type() == at::kBFloat16,
                "conv3x3: res must be a bf16 tensor on x's device");
    TORCH_CHECK(res->dim() == 4 && res->size(0) == NB && res->size(1) == K &&
                    res->size(2) == H && res->size(3) == W,
                "conv3x3: res must have the output's shape [N,K,H,W]");
    TORCH_CHECK(res->is_contiguous(at::MemoryFormat::ChannelsLast),
                "conv3x3: res channels_last expected");
  }
  auto out = at::empty({NB, K, H, W},
                       x.options().memory_format(at::MemoryFormat::ChannelsLast));
  const int64_t M = (int64_t)NB * H * W;
  // Row tiles per wave. Measured on MI355X (profiles/r2_conv3x3_micro.txt):
  // RT=1 (with its even/odd-kk dual chain) wins up to ~512k pixels, RT=2
  // wins at the largest M (1.2M); RT=4's occupancy drop (81 VGPRs -> 5
  // waves/SIMD) loses everywhere, so auto never picks it.
  const int rt = rtOverride > 0 ? (int)rtOverride : (M >= 512 * 1024) ? 2 : 1;
  const int64_t blocks = (M + 64 * rt - 1) / (64 * rt);
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  using conv3x3::bf16;
  auto bf = [](const c10::optional<at::Tensor>& t) -> const bf16* {
    return t.has_value() ? reinterpret_cast<const bf16*>(t->data_ptr()) : nullptr;
  };
  const bf16* xp = reinterpret_cast<const bf16*>(x.data_ptr());
  const bf16* wp = reinterpret_cast<const bf16*>(wPacked.data_ptr());
  bf16* op = reinterpret_cast<bf16*>(out.data_ptr());

  // Opt-in LDS band-slab variant (rtOverride<0 forces flat for micro A/Bs).
  static const bool ldsVariant = []() {
    const char* e = std::getenv("MOOLIB_AMD_CONV3_LDS");
    return e != nullptr && e[0] != '0';
  }();
  if (ldsVariant && rtOverride >= 0) {
    const int WS = W + 2;
    int BR = (int)(32768 / ((int64_t)WS * C * 2)) - 2;
    BR = std::min(BR, H);
    if (BR >= 4) {
      const size_t lds = (size_t)(BR + 2) * WS * C * 2;
      const int bandsPerImage = (H + BR - 1) / BR;
      const int64_t lblocks = (int64_t)NB * bandsPerImage;
#define C3_LDS_LAUNCH(CC, RIN)                                                       \
  hipLaunchKernelGGL((conv3x3::conv3x3_nhwc_lds_kernel<CC, RIN>), dim3(lblocks),     \
                     dim3(256), lds, stream, xp, wp, bf(biasIn), op, bf(bias1),      \
                     bf(res), bf(bias2), NB, H, W, (int)K, (int)epi, BR)
      if (C == 8) {
        if (reluIn) C3_LDS_LAUNCH(8, true); else C3_LDS_LAUNCH(8, false);
      } else if (C == 16) {
        if (reluIn) C3_LDS_LAUNCH(16, true); else C3_LDS_LAUNCH(16, false);
      } else {
        if (reluIn) C3_LDS_LAUNCH(32, true); else C3_LDS_LAUNCH(32, false);
      }
#undef C3_LDS_LAUNCH
      return out;
    }
  }
#define C3_LAUNCH(CC, RIN, RTT)                                                     \
  hipLaunchKernelGGL((conv3x3::conv3x3_nhwc_kernel<CC, RIN, RTT>), dim3(blocks),    \
                     dim3(256), 0, stream, xp, wp, bf(biasIn), op, bf(bias1),       \
                     bf(res), bf(bias2), NB, H, W, (int)K, (int)epi)
#define C3_RT(CC, RIN)                                                              \
  do {                                                                              \
    if (rt == 4) C3_LAUNCH(CC, RIN, 4);                                             \
    else if (rt == 2) C3_LAUNCH(CC, RIN, 2);                                        \
    else C3_LAUNCH(CC, RIN, 1);                                                     \
  } while (0)
  if (C == 8) {
    if (reluIn) C3_RT(8, true); else C3_RT(8, false);
  } else if (C == 16) {
    if (reluIn) C3_RT(16, true); else C3_RT(16, false);
  } else {
    if (reluIn) C3_RT(32, true); else C3_RT(32, false);
  }
#undef C3_RT
#undef C3_LAUNCH
  return out;
}
