// Register-resident masked LSTM scan for hidden sizes 128 and 512 (gfx950) —
// included by kernels.hip after lstm.hip.inc, whose fragment loaders it uses.
//
// The 256 kernel (lstm.hip.inc) keeps h, c and the whole pre-activation gate
// tile in LDS: 115.7 KB at H=256, about 230 KB at H=512, more than the 160 KB
// a workgroup can have. This family keeps in registers what can stay there,
// so that LDS holds only the MFMA A operand:
//   - one workgroup owns kBM batch rows for the whole sequence; nothing is
//     ever synchronised across workgroups;
//   - wave w owns kCT 16-column tiles of the hidden dimension and, for those
//     columns, all four gate tiles (i, f, g, o). mfma_f32_16x16x32_bf16 puts
//     D[row][col] of every tile in the same lane (col = lane&15,
//     row = (lane>>4)*4 + reg), so the gate nonlinearities, the cell update
//     and h = o*tanh(c) are lane-local on the accumulators: there is no gate
//     buffer and no gate phase;
//   - c (forward) and the running dh, dc (backward) live in registers for all
//     T steps;
//   - forward LDS is h as bf16, double-buffered: step t reads buffer t&1 and
//     writes the other, one __syncthreads() per step. Backward LDS is dG
//     (bf16, K = 4H), double-buffered the same way;
//   - the done mask multiplies the accumulator (nd * (h @ W)) and c. notdone
//     is 0 or 1, so this equals masking h before the product; nothing checks
//     it on the device;
//   - X[t], the saved gates and the cell states are read and written in the
//     D layout straight from global memory; at H=128 X[t] is requested before
//     the MFMA chain of its step and consumed after it;
//   - W_hh fragments stream from global memory (L2) in pack_mfma_b order;
//     nothing is cached in LDS.
//
// Row-tile height and wave count per hidden size (Geo<H>):
//   H=128: 32 rows,  8 waves, 1 column tile per wave ->  8 accumulator tiles
//   H=512: 16 rows, 16 waves, 2 column tiles per wave -> 8 accumulator tiles
// 16 rows at H=512 give R2D2's batch of 64 four workgroups, keep the
// accumulators at 32 VGPRs of the 128 a 1024-thread workgroup allows, and let
// the backward dG tile (16 x 2056 bf16 = 65.8 KB) fit twice.
//
// Rounding points: h to bf16 after each step (Hout, the LDS operand, hT);
// saved gates to bf16; dG to bf16 before the dG @ W_hh product and in dGout;
// dh0 to bf16. G = X + nd*(h@W) stays fp32 (the 256 kernel rounds it).

namespace lstm_wide {

using lstm::bf16;
using lstm::bf16x8;
using lstm::floatx4;
using lstm::loadAFrag;
using lstm::loadBFrag;
using lstm::sigmoidf;

// a * b as one single-lane v_mul_f32. These kernels are built to contain no
// packed fp32 instruction (v_pk_*_f32); the compiler pairs up runs of plain
// independent products, and the asm keeps it from seeing them.
DEV_INLINE float mulLane(float a, float b) {
  float r;
  asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

template <int H>
struct Geo;
template <>
struct Geo<128> {
  static constexpr int kBM = 32, kWaves = 8;
};
template <>
struct Geo<512> {
  static constexpr int kBM = 16, kWaves = 16;
};

// What the saving forward writes for the backward. The forward-only variant
// takes no pointers at all.
template <bool SAVE>
struct SavedOut {
  bf16* gates;  // [T, B, 4H] post-activation
  float* c;     // [T, B, H]
};
template <>
struct SavedOut<false> {};

template <int H, bool SAVE>
__global__ __launch_bounds__(Geo<H>::kWaves * 64) void lstm_wide_fwd_kernel(
    const bf16* __restrict__ X,          // [T, B, 4H]
    const float* __restrict__ notdone,   // [T, B], 0 or 1
    const bf16* __restrict__ h0,         // [B, H]
    const float* __restrict__ c0,        // [B, H]
    const bf16* __restrict__ whhPacked,  // packed [K=H, N=4H] fragments
    bf16* __restrict__ Hout,             // [T, B, H]
    SavedOut<SAVE> saved,
    bf16* __restrict__ hT,               // [B, H]
    float* __restrict__ cT,              // [B, H]
    int T, int B) {
  constexpr int kG = 4 * H;
  constexpr int kBM = Geo<H>::kBM;
  constexpr int kRT = kBM / 16;                    // row tiles per workgroup
  constexpr int kCT = H / 16 / Geo<H>::kWaves;     // hidden column tiles per wave
  constexpr int kHPad = H + 8;                     // LDS row padding (bank spread)
  __shared__ __attribute__((aligned(16))) bf16 hbuf[2][kBM][kHPad];

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int bm0 = blockIdx.x * kBM;
  const int col0 = wave * kCT * 16 + (lane & 15);  // + ct*16
  const int row0 = (lane >> 4) * 4;                // + rt*16 + reg

  float c[kCT][kRT][4];
#pragma unroll
  for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = rt * 16 + row0 + reg;
      const bool ok = bm0 + row < B;
#pragma unroll
      for (int ct = 0; ct < kCT; ++ct) {
        const int col = col0 + ct * 16;
        const int64_t o = (int64_t)(bm0 + row) * H + col;
        hbuf[0][row][col] = ok ? h0[o] : (bf16)0.f;
        c[ct][rt][reg] = ok ? c0[o] : 0.f;
      }
    }
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const bf16(*hin)[kHPad] = hbuf[t & 1];
    bf16(*hnext)[kHPad] = hbuf[(t & 1) ^ 1];

    // rows past B are computed on zeros and never stored
    float nd[kRT][4];
    bf16 x[4][kCT][kRT][4];
    auto loadRow = [&](int rt, int reg) {
      const int row = rt * 16 + row0 + reg;
      const bool ok = bm0 + row < B;
      const int64_t tb = (int64_t)t * B + bm0 + row;
      nd[rt][reg] = ok ? notdone[tb] : 0.f;
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int ct = 0; ct < kCT; ++ct)
          x[g][ct][rt][reg] = ok ? X[tb * kG + g * H + col0 + ct * 16] : (bf16)0.f;
    };
    // X[t] is requested ahead of the MFMA chain where the budget has room for
    // its 16*kCT*kRT registers (256 VGPRs at 512 threads); at 1024 threads
    // that spilled 44 B/lane, so H=512 loads each row where it is consumed
    constexpr bool kEarlyX = Geo<H>::kWaves <= 8;
    if constexpr (kEarlyX) {
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) loadRow(rt, reg);
    }

    // ---- h @ W_hh^T for this wave's columns of all four gates ----
    floatx4 acc[4][kCT][kRT];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int ct = 0; ct < kCT; ++ct)
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt) acc[g][ct][rt] = floatx4{0.f, 0.f, 0.f, 0.f};
    // not unrolled: one k-step already has 4*kCT fragment loads in flight
    // ahead of 4*kCT*kRT independent MFMA chains, and unrolling by 2 spilled
    // 100 B/lane at H=512 (128-VGPR budget at 1024 threads)
#pragma unroll 1
    for (int kk = 0; kk < H / 32; ++kk) {
      bf16x8 a[kRT];
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt) a[rt] = loadAFrag<kHPad>(hin, rt * 16, kk * 32, lane);
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int ct = 0; ct < kCT; ++ct) {
          const bf16x8 b = loadBFrag(whhPacked, g * (H / 16) + wave * kCT + ct, kk, H / 32, lane);
#pragma unroll
          for (int rt = 0; rt < kRT; ++rt)
            acc[g][ct][rt] =
                __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[rt], b, acc[g][ct][rt], 0, 0, 0);
        }
    }

    // ---- gates, cell update and h on the accumulators ----
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        if constexpr (!kEarlyX) loadRow(rt, reg);
        const int row = rt * 16 + row0 + reg;
        const bool ok = bm0 + row < B;
        const int64_t tb = (int64_t)t * B + bm0 + row;
        const float m = nd[rt][reg];
#pragma unroll
        for (int ct = 0; ct < kCT; ++ct) {
          const int col = col0 + ct * 16;
          const float gi = sigmoidf(fmaf(m, acc[0][ct][rt][reg], (float)x[0][ct][rt][reg]));
          const float gf = sigmoidf(fmaf(m, acc[1][ct][rt][reg], (float)x[1][ct][rt][reg]));
          const float gg = tanhf(fmaf(m, acc[2][ct][rt][reg], (float)x[2][ct][rt][reg]));
          const float go = sigmoidf(fmaf(m, acc[3][ct][rt][reg], (float)x[3][ct][rt][reg]));
          const float cn = fmaf(gf, m * c[ct][rt][reg], gi * gg);
          const bf16 hn = (bf16)(go * tanhf(cn));
          c[ct][rt][reg] = cn;
          hnext[row][col] = hn;
          if (ok) {
            Hout[tb * H + col] = hn;
            if constexpr (SAVE) {
              saved.c[tb * H + col] = cn;
              bf16* gp = saved.gates + tb * kG + col;
              gp[0] = (bf16)gi;
              gp[H] = (bf16)gf;
              gp[2 * H] = (bf16)gg;
              gp[3 * H] = (bf16)go;
            }
          }
        }
      }
    // the only barrier of the step: hnext is complete before step t+1 reads
    // it, and every read of hin is done before step t+1 overwrites it
    __syncthreads();
  }

  // each lane reads back the h it wrote itself (or h0 when T == 0)
  const bf16(*hlast)[kHPad] = hbuf[T & 1];
#pragma unroll
  for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = rt * 16 + row0 + reg;
      if (bm0 + row < B) {
#pragma unroll
        for (int ct = 0; ct < kCT; ++ct) {
          const int col = col0 + ct * 16;
          const int64_t o = (int64_t)(bm0 + row) * H + col;
          hT[o] = hlast[row][col];
          cT[o] = c[ct][rt][reg];
        }
      }
    }
}

template <int H>
__global__ __launch_bounds__(Geo<H>::kWaves * 64) void lstm_wide_bwd_kernel(
    const bf16* __restrict__ gates,       // [T, B, 4H] post-activation
    const float* __restrict__ cOut,       // [T, B, H]
    const float* __restrict__ c0,         // [B, H]
    const float* __restrict__ notdone,    // [T, B], 0 or 1
    const bf16* __restrict__ dH,          // [T, B, H] incoming grad on H
    const bf16* __restrict__ dhT,         // [B, H] grad on final h (may be null)
    const float* __restrict__ dcT,        // [B, H] grad on final c (may be null)
    const bf16* __restrict__ whhPackedN,  // packed [K=4H, N=H] fragments
    bf16* __restrict__ dGout,             // [T, B, 4H]
    bf16* __restrict__ dh0,               // [B, H]
    float* __restrict__ dc0,              // [B, H]
    int T, int B) {
  constexpr int kG = 4 * H;
  constexpr int kBM = Geo<H>::kBM;
  constexpr int kRT = kBM / 16;
  constexpr int kCT = H / 16 / Geo<H>::kWaves;
  constexpr int kGPad = kG + 8;
  // dG of step t in buffer t&1
  __shared__ __attribute__((aligned(16))) bf16 dgbuf[2][kBM][kGPad];

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int bm0 = blockIdx.x * kBM;
  const int col0 = wave * kCT * 16 + (lane & 15);
  const int row0 = (lane >> 4) * 4;

  // running gradients carried into step t, for the (row, col) this lane owns
  float dh[kCT][kRT][4], dc[kCT][kRT][4];
#pragma unroll
  for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = rt * 16 + row0 + reg;
      const bool ok = bm0 + row < B;
#pragma unroll
      for (int ct = 0; ct < kCT; ++ct) {
        const int64_t o = (int64_t)(bm0 + row) * H + col0 + ct * 16;
        dh[ct][rt][reg] = (ok && dhT) ? (float)dhT[o] : 0.f;
        dc[ct][rt][reg] = (ok && dcT) ? dcT[o] : 0.f;
      }
    }

  for (int t = T - 1; t >= 0; --t) {
    bf16(*dg)[kGPad] = dgbuf[t & 1];
    float nd[kRT][4];

    // ---- gate gradients -> dG (pre-activation), lane-local ----
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = rt * 16 + row0 + reg;
        const bool ok = bm0 + row < B;
        const int64_t tb = (int64_t)t * B + bm0 + row;
        const float m = ok ? notdone[tb] : 0.f;
        nd[rt][reg] = m;
#pragma unroll
        for (int ct = 0; ct < kCT; ++ct) {
          const int col = col0 + ct * 16;
          const int64_t o = tb * H + col;
          const bf16* gp = gates + tb * kG + col;
          const float gi = ok ? (float)gp[0] : 0.f;
          const float gf = ok ? (float)gp[H] : 0.f;
          const float gg = ok ? (float)gp[2 * H] : 0.f;
          const float go = ok ? (float)gp[3 * H] : 0.f;
          const float cn = ok ? cOut[o] : 0.f;
          float cprev = 0.f;
          if (ok) cprev = (t == 0) ? c0[(int64_t)(bm0 + row) * H + col] : cOut[o - (int64_t)B * H];
          const float cm = m * cprev;  // c_masked at step t
          const float dht = dh[ct][rt][reg] + (ok ? (float)dH[o] : 0.f);
          const float tc = tanhf(cn);
          const float dcn = dc[ct][rt][reg] + dht * go * (1.f - tc * tc);
          const bf16 dgi = (bf16)(dcn * gg * gi * (1.f - gi));
          const bf16 dgf = (bf16)(dcn * cm * gf * (1.f - gf));
          const bf16 dgg = (bf16)(dcn * gi * (1.f - gg * gg));
          const bf16 dgo = (bf16)(dht * tc * go * (1.f - go));
          dg[row][col] = dgi;
          dg[row][H + col] = dgf;
          dg[row][2 * H + col] = dgg;
          dg[row][3 * H + col] = dgo;
          // carry into t-1 (the mask applies to both the h and the c chain)
          dc[ct][rt][reg] = m * gf * dcn;
          if (ok) {
            bf16* op = dGout + tb * kG + col;
            op[0] = dgi;
            op[H] = dgf;
            op[2 * H] = dgg;
            op[3 * H] = dgo;
          }
        }
      }
    // the only barrier of the step: dg is complete before the product reads
    // it; step t-1 writes the other buffer, and step t-2 reuses this one only
    // after every wave has passed the barrier of step t-1
    __syncthreads();

    // ---- dh_{t-1} = nd * (dG @ W_hh), for this wave's hidden columns ----
    floatx4 acc[kCT][kRT];
#pragma unroll
    for (int ct = 0; ct < kCT; ++ct)
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt) acc[ct][rt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int kk = 0; kk < kG / 32; ++kk) {
      bf16x8 a[kRT];
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt) a[rt] = loadAFrag<kGPad>(dg, rt * 16, kk * 32, lane);
#pragma unroll
      for (int ct = 0; ct < kCT; ++ct) {
        const bf16x8 b = loadBFrag(whhPackedN, wave * kCT + ct, kk, kG / 32, lane);
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt)
          acc[ct][rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[rt], b, acc[ct][rt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int ct = 0; ct < kCT; ++ct)
#pragma unroll
      for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          dh[ct][rt][reg] = mulLane(nd[rt][reg], acc[ct][rt][reg]);
  }

#pragma unroll
  for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = rt * 16 + row0 + reg;
      if (bm0 + row < B) {
#pragma unroll
        for (int ct = 0; ct < kCT; ++ct) {
          const int64_t o = (int64_t)(bm0 + row) * H + col0 + ct * 16;
          dh0[o] = (bf16)dh[ct][rt][reg];
          dc0[o] = dc[ct][rt][reg];
        }
      }
    }
}

}  // namespace lstm_wide
