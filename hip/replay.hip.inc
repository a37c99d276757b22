// Device-side prioritized replay for gfx950 — included by kernels.hip (after
// the batched-copy section, whose descriptor limit it shares).
//
// Three small latency-bound kernels, so that adding, sampling and
// re-prioritising are a fixed number of launches whatever the capacity and
// the number of nest leaves, and none of them needs the host to wait:
//
//   replay_tree_update  leaves <- priority^alpha, ancestors recomputed level
//                       by level, max_priority raised;
//   replay_tree_sample  stratified descent of the sum tree + normalised
//                       importance weights;
//   replay_rows         gather / scatter of whole items of every leaf of a
//                       nest by a device-resident index (batch- or time-major).
//
// Sum tree: L = capacity rounded up to a power of two, tree is float32[2L],
// tree[1] the root, tree[L + slot] the leaves, tree[0] unused and every
// internal node EXACTLY fl32(tree[2n] + tree[2n+1]). The tree is therefore a
// pure function of its leaves, and the plain-torch path of
// moolib_amd/ops/replay.py, which performs the same operations in the same
// order, reproduces it bit for bit.
//
// The tree kernels are ONE workgroup each: threads stride over the K slots /
// B draws and workgroup barriers order the phases. No atomics; all stores are
// ordinary vector stores. IEEE division, no fast intrinsics, fp contraction
// off; the two pows run in double and are rounded to fp32 once.

namespace replay {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kWave;
// Most slots one replay_tree_update launch takes; the Python op chunks longer
// lists in order, so the last occurrence of a slot still wins.
constexpr int kMaxUpdate = 4096;
// Largest batch of replay_tree_sample (its unnormalised weights wait in LDS,
// 8 B each, for the batch maximum). Larger batches are rejected on the host.
constexpr int kMaxSample = 4096;

// Every thread receives the block maximum. `red` holds kWaves elements.
template <typename T>
DEV_INLINE T blockAllMax(T v, T* red) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    T o = __shfl_down(v, off);
    v = o > v ? o : v;
  }
  const int lane = threadIdx.x % kWave;
  const int wave = threadIdx.x / kWave;
  if (lane == 0) red[wave] = v;
  __syncthreads();
  T m = red[0];
  for (int w = 1; w < kWaves; ++w) m = red[w] > m ? red[w] : m;
  __syncthreads();  // red may be reused
  return m;
}

// tree and max_priority are read and written across barriers: no __restrict__.
__global__ __launch_bounds__(kThreads) void replay_tree_update_kernel(
    float* tree,                           // [2L]
    float* max_priority,                   // [1]
    const int64_t* __restrict__ slots,     // [K]
    const float* __restrict__ priorities,  // [K] or null: enter at max_priority
    int K, double alpha, int64_t L, int levels) {
  __shared__ int64_t sSlot[kThreads];
  __shared__ float sRed[kWaves];
  const int tid = threadIdx.x;
  const float oldMax = max_priority[0];
  float rawMax = oldMax;

  // ---- leaves. Rounds of kThreads slots, in order, a barrier between rounds:
  // a later round overwrites an earlier one. Inside a round a thread writes
  // only if no later thread of the round holds the same slot (last wins).
  for (int base = 0; base < K; base += kThreads) {
    const int k = base + tid;
    const int n = min(kThreads, K - base);
    int64_t slot = -1;
    float p = oldMax;
    if (k < K) {
      slot = slots[k];
      // Defensive: a corrupted slot must not write out of bounds.
      if (slot < 0 || slot >= L) slot = -1;
      if (priorities != nullptr) p = priorities[k];
    }
    sSlot[tid] = slot;
    __syncthreads();
    if (slot >= 0) {
      bool last = true;
      for (int j = tid + 1; j < n; ++j) {
        if (sSlot[j] == slot) {
          last = false;
          break;
        }
      }
      if (last) tree[L + slot] = (float)pow((double)fmaxf(p, 1e-6f), alpha);
      rawMax = fmaxf(rawMax, p);
    }
    __syncthreads();
  }

  // ---- ancestors, one level per barrier. Two slots under the same parent
  // recompute it from the same two children to the same value.
  for (int lv = 1; lv <= levels; ++lv) {
    for (int k = tid; k < K; k += kThreads) {
      const int64_t slot = slots[k];
      if (slot < 0 || slot >= L) continue;
      const int64_t node = (L + slot) >> lv;
      tree[node] = tree[2 * node] + tree[2 * node + 1];
    }
    __syncthreads();
  }

  if (priorities != nullptr) {
    const float m = blockAllMax<float>(rawMax, sRed);
    if (tid == 0) max_priority[0] = fmaxf(oldMax, m);
  }
}

__global__ __launch_bounds__(kThreads) void replay_tree_sample_kernel(
    const float* __restrict__ tree,  // [2L]
    const float* __restrict__ u,     // [B] in [0, 1)
    int64_t* __restrict__ idx,       // [B]
    float* __restrict__ weights,     // [B]
    int B, int64_t L, double size, double negBeta) {
#pragma clang fp contract(off)
  __shared__ double sW[kMaxSample];
  __shared__ double sRed[kWaves];
  const int tid = threadIdx.x;
  const float total = tree[1];
  const float seg = total / (float)B;
  double wmax = 0.0;
  for (int b = tid; b < B; b += kThreads) {
    float target = ((float)b + u[b]) * seg;
    int64_t node = 1;
    while (node < L) {
      const int64_t left = 2 * node;
      const float tl = tree[left];
      const float tr = tree[left + 1];
      // Never step into an empty subtree, even when rounding pushed target
      // to `total` or a tiny leaf was swamped by a huge neighbour.
      if (tr > 0.f && (target >= tl || tl == 0.f)) {
        target = target - tl;
        node = left + 1;
      } else {
        node = left;
      }
    }
    idx[b] = node - L;
    const double w = pow(size * (double)tree[node] / (double)total, negBeta);
    sW[b] = w;
    wmax = fmax(wmax, w);
  }
  wmax = blockAllMax<double>(wmax, sRed);
  for (int b = tid; b < B; b += kThreads) weights[b] = (float)(sW[b] / wmax);
}

// One leaf of a nest: N items of `rows` rows of `inner` bytes; an item of
// index i starts at i * itemStride, its row t at t * rowStride further on.
struct RowsDesc {
  const uint8_t* src;
  uint8_t* dst;
  int64_t rows;
  int64_t inner;
  int64_t srcItemStride;
  int64_t srcRowStride;
  int64_t dstItemStride;
  int64_t dstRowStride;
  int32_t vec;  // 16 / 4 / 1: granularity valid for ptrs, strides and inner
  int32_t pad;
};

struct RowsPack {
  RowsDesc d[kMaxCopyDescs];  // 24 * 72 B, with the tail well under the 4 KB arg limit
  const int64_t* index;       // [N], on the device
  int64_t n_items;
  int64_t limit;    // valid index values are [0, limit)
  int32_t n;
  int32_t scatter;  // 0: index picks the source item; 1: the destination item
};

template <typename V>
DEV_INLINE void rowsRun(const RowsDesc& e, const RowsPack& pack, int64_t start, int64_t step) {
  const int64_t perRow = e.inner / (int64_t)sizeof(V);
  const int64_t perItem = e.rows * perRow;
  const int64_t total = pack.n_items * perItem;
  for (int64_t unit = start; unit < total; unit += step) {
    const int64_t item = unit / perItem;
    const int64_t rem = unit - item * perItem;
    const int64_t t = rem / perRow;
    const int64_t col = (rem - t * perRow) * (int64_t)sizeof(V);
    const int64_t i = pack.index[item];
    // Defensive: an index outside the storage neither reads nor writes.
    if (i < 0 || i >= pack.limit) continue;
    const int64_t si = pack.scatter ? item : i;
    const int64_t di = pack.scatter ? i : item;
    *reinterpret_cast<V*>(e.dst + di * e.dstItemStride + t * e.dstRowStride + col) =
        *reinterpret_cast<const V*>(e.src + si * e.srcItemStride + t * e.srcRowStride + col);
  }
}

__global__ void replay_rows_kernel(RowsPack pack) {
  const RowsDesc& e = pack.d[blockIdx.y];
  const int64_t start = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  if (e.vec == 16) rowsRun<uint4>(e, pack, start, step);
  else if (e.vec == 4) rowsRun<uint32_t>(e, pack, start, step);
  else rowsRun<uint8_t>(e, pack, start, step);
}

inline void checkTree(const at::Tensor& tree, int64_t L, const char* fn) {
  TORCH_CHECK(tree.defined() && tree.is_cuda() && tree.scalar_type() == at::kFloat &&
                  tree.dim() == 1 && tree.is_contiguous(),
              fn, ": tree must be a contiguous float32 CUDA vector");
  TORCH_CHECK(L >= 1 && (L & (L - 1)) == 0 && tree.numel() == 2 * L, fn,
              ": tree must have 2L elements with L a power of two, got L = ", L, " and ",
              tree.numel(), " elements");
}

inline int log2Of(int64_t L) {
  int levels = 0;
  while (((int64_t)1 << levels) < L) ++levels;
  return levels;
}

}  // namespace replay

// Leaves tree[L + slots[k]] <- max(p_k, 1e-6)^alpha (the last occurrence of a
// slot wins), ancestors recomputed, max_priority <- max(old, max_k p_k).
// Without `priorities`, p_k is the current max_priority.
void replay_tree_update(at::Tensor tree, at::Tensor max_priority, at::Tensor slots,
                        c10::optional<at::Tensor> priorities, double alpha, int64_t L) {
  replay::checkTree(tree, L, "replay_tree_update");
  TORCH_CHECK(max_priority.defined() && max_priority.is_cuda() &&
                  max_priority.device() == tree.device() &&
                  max_priority.scalar_type() == at::kFloat && max_priority.numel() == 1,
              "replay_tree_update: max_priority must be a 1-element float32 tensor on the "
              "tree's device");
  TORCH_CHECK(slots.defined() && slots.is_cuda() && slots.device() == tree.device() &&
                  slots.scalar_type() == at::kLong && slots.dim() == 1 && slots.is_contiguous(),
              "replay_tree_update: slots must be a contiguous int64 vector on the tree's device");
  const int64_t K = slots.numel();
  TORCH_CHECK(K <= replay::kMaxUpdate, "replay_tree_update: ", K, " slots exceed the limit of ",
              replay::kMaxUpdate, " per launch");
  const float* prio = nullptr;
  if (priorities.has_value() && priorities->defined()) {
    const at::Tensor& p = *priorities;
    TORCH_CHECK(p.is_cuda() && p.device() == tree.device() && p.scalar_type() == at::kFloat &&
                    p.dim() == 1 && p.numel() == K && p.is_contiguous(),
                "replay_tree_update: priorities must be a contiguous float32 vector as long as "
                "slots, on the tree's device");
    prio = p.data_ptr<float>();
  }
  if (K == 0) return;
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(replay::replay_tree_update_kernel, dim3(1), dim3(replay::kThreads), 0, stream,
                     tree.data_ptr<float>(), max_priority.data_ptr<float>(),
                     slots.data_ptr<int64_t>(), prio, (int)K, alpha, L, replay::log2Of(L));
}

// Stratified sample of B = u.numel() slots and their importance weights
// (size * p / total)^-beta / max. `idx_out` / `weights_out`, if given, are
// the [B] buffers written into (every element).
std::vector<at::Tensor> replay_tree_sample(at::Tensor tree, int64_t L, int64_t size, at::Tensor u,
                                           double beta, c10::optional<at::Tensor> idx_out,
                                           c10::optional<at::Tensor> weights_out) {
  replay::checkTree(tree, L, "replay_tree_sample");
  TORCH_CHECK(size >= 1 && size <= L, "replay_tree_sample: size must be in [1, L], got ", size);
  TORCH_CHECK(u.defined() && u.is_cuda() && u.device() == tree.device() &&
                  u.scalar_type() == at::kFloat && u.dim() == 1 && u.is_contiguous(),
              "replay_tree_sample: u must be a contiguous float32 vector on the tree's device");
  const int64_t B = u.numel();
  TORCH_CHECK(B >= 1 && B <= replay::kMaxSample, "replay_tree_sample: batch size must be in [1, ",
              replay::kMaxSample, "], got ", B);
  at::Tensor idx, weights;
  if (idx_out.has_value() && idx_out->defined()) {
    idx = *idx_out;
    TORCH_CHECK(idx.is_cuda() && idx.device() == tree.device() && idx.scalar_type() == at::kLong &&
                    idx.dim() == 1 && idx.numel() == B && idx.is_contiguous(),
                "replay_tree_sample: idx_out must be a contiguous int64 [B] tensor");
  } else {
    idx = at::empty({B}, u.options().dtype(at::kLong));
  }
  if (weights_out.has_value() && weights_out->defined()) {
    weights = *weights_out;
    TORCH_CHECK(weights.is_cuda() && weights.device() == tree.device() &&
                    weights.scalar_type() == at::kFloat && weights.dim() == 1 &&
                    weights.numel() == B && weights.is_contiguous(),
                "replay_tree_sample: weights_out must be a contiguous float32 [B] tensor");
  } else {
    weights = at::empty({B}, u.options());
  }
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(replay::replay_tree_sample_kernel, dim3(1), dim3(replay::kThreads), 0, stream,
                     tree.data_ptr<float>(), u.data_ptr<float>(), idx.data_ptr<int64_t>(),
                     weights.data_ptr<float>(), (int)B, L, (double)size, -beta);
  return {idx, weights};
}

// Whole items of every leaf moved by a device-resident index, all leaves in
// one launch (chunked by kMaxCopyDescs). storage[i] is [capacity, *item],
// other[i] holds N = index.numel() items, batch-major [N, *item] or
// time-major [item[0], N, *item[1:]] (0-dim items: [N] either way).
//   mode 0: other[b]    = storage[index[b]]       mode 1: other[t, b] = storage[index[b], t]
//   mode 2: storage[index[k]] = other[k]          mode 3: storage[index[k], t] = other[t, k]
// Scatter indices must be unique. Nothing is read back.
void replay_rows(std::vector<at::Tensor> storage, std::vector<at::Tensor> other, at::Tensor index,
                 int64_t mode) {
  TORCH_CHECK(storage.size() == other.size(), "replay_rows: length mismatch");
  TORCH_CHECK(mode >= 0 && mode <= 3, "replay_rows: mode must be 0..3, got ", mode);
  TORCH_CHECK(index.defined() && index.is_cuda() && index.scalar_type() == at::kLong &&
                  index.dim() == 1 && index.is_contiguous(),
              "replay_rows: index must be a contiguous int64 CUDA vector");
  const int64_t N = index.numel();
  const bool scatter = mode >= 2;
  const bool timeMajor = (mode & 1) != 0;
  if (storage.empty()) return;
  TORCH_CHECK(storage[0].defined() && storage[0].dim() >= 1,
              "replay_rows: storage leaves must be [capacity, ...]");
  const int64_t capacity = storage[0].size(0);

  replay::RowsPack pack;
  pack.index = index.data_ptr<int64_t>();
  pack.n_items = N;
  pack.limit = capacity;
  pack.n = 0;
  pack.scatter = scatter ? 1 : 0;
  int64_t maxUnits = 0;
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  auto flush = [&]() {
    if (pack.n == 0) return;
    const int threads = 256;
    const int64_t blocksX = std::min<int64_t>((maxUnits + threads - 1) / threads, 1024);
    hipLaunchKernelGGL(replay::replay_rows_kernel, dim3(blocksX, pack.n), dim3(threads), 0, stream,
                       pack);
    pack.n = 0;
    maxUnits = 0;
  };
  // validate everything before the first launch
  for (size_t i = 0; i < storage.size(); ++i) {
    const at::Tensor& s = storage[i];
    const at::Tensor& o = other[i];
    TORCH_CHECK(s.defined() && o.defined() && s.is_cuda() && o.is_cuda() &&
                    s.device() == index.device() && o.device() == index.device(),
                "replay_rows: leaf ", i, " must be on the index's CUDA device");
    TORCH_CHECK(s.scalar_type() == o.scalar_type(), "replay_rows: leaf ", i, " dtype mismatch: ",
                s.scalar_type(), " vs ", o.scalar_type());
    TORCH_CHECK(s.is_contiguous() && o.is_contiguous(), "replay_rows: leaf ", i,
                " must be contiguous");
    TORCH_CHECK(s.dim() >= 1 && s.size(0) == capacity, "replay_rows: storage leaf ", i,
                " must be [", capacity, ", ...], got ", s.sizes());
    std::vector<int64_t> want(s.sizes().begin(), s.sizes().end());
    want[0] = N;
    if (timeMajor && s.dim() >= 2) std::swap(want[0], want[1]);
    TORCH_CHECK(o.sizes() == at::IntArrayRef(want), "replay_rows: leaf ", i, " must have shape ",
                at::IntArrayRef(want), ", got ", o.sizes());
  }
  if (N == 0) return;
  for (size_t i = 0; i < storage.size(); ++i) {
    const at::Tensor& s = storage[i];
    const at::Tensor& o = other[i];
    const int64_t itemBytes = (s.numel() / capacity) * s.element_size();
    if (itemBytes == 0) continue;
    replay::RowsDesc e;
    int64_t oItem, oRow;
    if (timeMajor && s.dim() >= 2) {
      e.rows = s.size(1);
      e.inner = itemBytes / e.rows;
      oItem = e.inner;
      oRow = N * e.inner;
    } else {  // a batch-major item is one contiguous row
      e.rows = 1;
      e.inner = itemBytes;
      oItem = itemBytes;
      oRow = itemBytes;
    }
    const uint8_t* sp = (const uint8_t*)s.data_ptr();
    const uint8_t* op = (const uint8_t*)o.data_ptr();
    e.src = scatter ? op : sp;
    e.dst = const_cast<uint8_t*>(scatter ? sp : op);
    e.srcItemStride = scatter ? oItem : itemBytes;
    e.srcRowStride = scatter ? oRow : e.inner;
    e.dstItemStride = scatter ? itemBytes : oItem;
    e.dstRowStride = scatter ? e.inner : oRow;
    // as vecWidthFor, over both pointers, the row and all four strides
    auto ok = [&](int64_t v) {
      return ((uintptr_t)sp % v == 0) && ((uintptr_t)op % v == 0) && (e.inner % v == 0) &&
             (e.srcItemStride % v == 0) && (e.srcRowStride % v == 0) &&
             (e.dstItemStride % v == 0) && (e.dstRowStride % v == 0);
    };
    e.vec = ok(16) ? 16 : (ok(4) ? 4 : 1);
    e.pad = 0;
    pack.d[pack.n++] = e;
    maxUnits = std::max(maxUnits, N * itemBytes / e.vec);
    if (pack.n == kMaxCopyDescs) flush();
  }
  flush();
}
