// per_kernels.hip — prioritized experience replay on the device: the sum / min
// segment trees, the CPython-exact proportional draw with its importance-
// sampling weights, and the priority updates (insert, explicit leaves, TD
// errors).
//
// The reference's replay/prioritized_replay.py + replay/segment_tree.py cannot
// be constructed (its super() names another class, it reads self._storage, and
// sample returns only the experiences), so there is no reference run to match.
// The semantics are those of its text read as the openai/baselines code it was
// adapted from, with these decisions:
//
//  1. Trees.  cap = the smallest power of two >= memory_size.  Sum tree and min
//     tree are fp64 (the reference's are Python floats).  Node i has children
//     2i and 2i+1, the leaf of slot s is node cap + s.  A parent is always
//     left + right (resp. min(left, right)) recomputed from its two children,
//     so every tree value is bit-identical to the Python tree's.  Empty leaves
//     are 0.0 (sum) and +inf (min).  max_priority starts at 1.0.
//     Layout: 4 * cap doubles, node i = the pair {sum, min} at [2i], [2i+1];
//     node 0 is unused and [0] holds max_priority.
//  2. Insert.  The slot that is written gets leaf max_priority ** alpha, as in
//     baselines (the reference text assigns it to the slot after the one
//     written: a transcription slip of a class that never ran, not kept).  A
//     bulk insert of n > memory_size rows touches only the surviving slots.
//  3. Draw.  For each sample in stream order: mass = random.random() * total,
//     idx = find_prefixsum_idx(mass).  total = sum_tree.sum(0, len - 1), which
//     by the tree's reduce (it subtracts one from `end`) is the sum over slots
//     0 .. len-2: slot len-1 is left out of the mass and never drawn
//     (baselines' behaviour, kept).  total is evaluated in the order of the
//     recursive reduce: on the way from the root to leaf len-2 every step to
//     the right collects the left child's value, the node whose range ends at
//     len-2 contributes its own, and the terms are summed from the deepest to
//     the shallowest.  random.random() is CPython's: a = genrand_uint32() >> 5,
//     b = genrand_uint32() >> 6, (a * 67108864.0 + b) / 2^53: exactly two
//     words per draw, no rejection.  Descent: at node i < cap, go left if
//     sum[2i] > mass, else mass -= sum[2i] and go right.  The result is
//     clamped to len - 1 (the reference would raise IndexError; only a
//     rounding coincidence reaches it).  len < 2 is an argument error.
//  4. IS weights.  p_min = min_tree.min() / sum_tree.sum() over the whole
//     tree, max_w = (p_min * len) ** (-beta), w_i = (leaf[idx_i] /
//     sum_tree.sum() * len) ** (-beta) / max_w, in fp64, stored as float32;
//     beta = 0 gives exactly 1.0f.
//  5. Priority update.  update_priorities has the sequential loop's meaning:
//     where an index repeats the LAST occurrence wins; max_priority =
//     max(max_priority, every priority).  From TD errors priority = |td| + eps
//     (eps > 0), leaf = priority ** alpha in fp64.
//
// Both kernels are single-workgroup.  The update walks log2(cap) levels with a
// workgroup barrier between them: one CU's own stores and loads are coherent
// at workgroup scope, where a walk split over workgroups would pay an
// agent-scope release (an L2 writeback) per level.
#include <math.h>
#include "smi_device.hpp"
#include "smi_internal.hpp"
#include "mt19937.hpp"

namespace smi {

constexpr int kPerUpd = 4096;              // indices per update launch
constexpr int kPerE = kPerUpd / kMtWG;     // per thread
constexpr int kPerTop = 2048;              // sum-tree nodes [1, kPerTop) kept in LDS by the draw
constexpr int kPerChunk = 2048;            // draws per pass of the draw kernel (2 words each)
enum { PER_SET = 0, PER_INSERT = 1, PER_TD = 2 };

// ----------------------------------------------------------- shared pieces
// CPython's random.random() from two consecutive tempered words
__host__ __device__ inline double per_u53(uint32_t w0, uint32_t w1) {
  const uint32_t a = w0 >> 5, b = w1 >> 6;
  return ((double)a * 67108864.0 + (double)b) * (1.0 / 9007199254740992.0);
}

// node whose range ends at leaf `end` on the reduce's way down: the highest
// ancestor-or-self of the leaf that has it as its rightmost leaf
__host__ __device__ inline int64_t per_reduce_stop(int64_t cap, int64_t end) {
  int64_t node = cap + end;
  while (node > 1 && (node & 1)) node >>= 1;
  return node;
}

__host__ __device__ inline float per_weight(double leaf, double sum, double max_w, int64_t len,
                                            double beta) {
  if (beta == 0.0) return 1.0f;
  return (float)(pow(leaf / sum * (double)len, -beta) / max_w);
}

// ------------------------------------------------------------------ host
int per_init_host(double* tree, int64_t cap) {
  tree[0] = 1.0;
  tree[1] = 0.0;
  for (int64_t i = 1; i < 2 * cap; ++i) {
    tree[2 * i] = 0.0;
    tree[2 * i + 1] = INFINITY;
  }
  return SMI_OK;
}

int per_set_host(double* tree, int64_t cap, const int64_t* idx, const double* leaf, int64_t n) {
  for (int64_t i = 0; i < n; ++i) {
    const int64_t node = cap + idx[i];
    tree[2 * node] = tree[2 * node + 1] = leaf[i];
  }
  for (int64_t i = 0; i < n; ++i)
    for (int64_t node = (cap + idx[i]) >> 1; node >= 1; node >>= 1) {
      const double* l = tree + 4 * node;
      tree[2 * node] = l[0] + l[2];
      tree[2 * node + 1] = l[3] < l[1] ? l[3] : l[1];
    }
  return SMI_OK;
}

static double per_total_host(const double* tree, int64_t cap, int64_t len) {
  int64_t node = per_reduce_stop(cap, len - 2);
  double acc = tree[2 * node];
  for (; node > 1; node >>= 1)
    if (node & 1) acc = tree[2 * (node - 1)] + acc;
  return acc;
}

int per_sample_host(const double* tree, int64_t cap, int64_t len, uint32_t* st, int64_t batch,
                    double beta, int64_t* idx_out, float* w_out) {
  const double total = per_total_host(tree, cap, len);
  const double sum = tree[2], p_min = tree[3] / sum;
  const double max_w = pow(p_min * (double)len, -beta);
  for (int64_t b = 0; b < batch; ++b) {
    const uint32_t w0 = mt_next_host(st), w1 = mt_next_host(st);
    double mass = per_u53(w0, w1) * total;
    int64_t i = 1;
    while (i < cap) {
      const double s = tree[4 * i];
      if (s > mass) i = 2 * i;
      else { mass -= s; i = 2 * i + 1; }
    }
    int64_t slot = i - cap;
    if (slot > len - 1) slot = len - 1;
    idx_out[b] = slot;
    w_out[b] = per_weight(tree[2 * (cap + slot)], sum, max_w, len, beta);
  }
  return SMI_OK;
}

// ---------------------------------------------------------------- device
__global__ void __launch_bounds__(kWG)
per_init_kernel(double2* __restrict__ nodes, int64_t n2) {
  for (int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x; i < n2; i += (int64_t)gridDim.x * kWG)
    nodes[i] = i ? make_double2(0.0, INFINITY) : make_double2(1.0, 0.0);
}

int launch_per_init(double* tree, int64_t cap, hipStream_t s) {
  const int64_t n2 = 2 * cap;
  int64_t g = (n2 + kWG - 1) / kWG;
  if (g > 2048) g = 2048;
  hipLaunchKernelGGL(per_init_kernel, dim3((int)g), dim3(kWG), 0, s,
                     reinterpret_cast<double2*>(tree), n2);
  return check_launch("per_init_kernel");
}

__device__ __forceinline__ double block_max_d(double v, double* scratch) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) scratch[wave] = v;
  __syncthreads();
  double m = scratch[0];
#pragma unroll
  for (int w = 1; w < kMtWG / 64; ++w) m = fmax(m, scratch[w]);
  __syncthreads();
  return m;
}

// One workgroup, n <= kPerUpd leaves: PER_SET leaf[e] at slot idx[e]; PER_INSERT
// max_priority ** alpha at the ring slots (first_slot + e) % memory_size (all
// distinct); PER_TD (|td[e]| + eps) ** alpha at slot idx[e], and max_priority
// raised to the largest priority.  Where a slot repeats only its last
// occurrence writes (the sequential loop's result): every element enters
// (slot, e) into an LDS hash table (open addressing, 2^hbits >= 2n cells, one
// 64-bit cell = slot + 1 above 13 bits of e, so an atomic max on a slot's cell
// keeps its largest e) and stays live iff the cell ends with its own e.  A live
// thread then recomputes node (cap + slot) >> level from the node's two
// children level by level, a workgroup barrier between levels; threads that
// share a node store identical values.  Once a level has kMtWG nodes the walk
// through L2 stops: that level is loaded into LDS, the ten levels above it are
// finished there and stored back (every node of them, dirty or not: a parent
// is a pure function of its children).  The tree is neither const nor
// restrict: every level reads what the level below stored.
// Dynamic LDS: per_update_lds(hbits) bytes = the table, reused for the top
// levels, then kMtWG / 64 doubles of reduction scratch.
typedef unsigned long long u64;
constexpr int kPerTopBytes = 2 * kMtWG * (int)sizeof(double2);
__host__ __device__ inline size_t per_update_main(int hbits) {
  const size_t t = hbits ? ((size_t)8 << hbits) : 0;
  return t > (size_t)kPerTopBytes ? t : (size_t)kPerTopBytes;
}
inline size_t per_update_lds(int hbits) { return per_update_main(hbits) + (kMtWG / 64) * sizeof(double); }

template <int MODE>
__global__ void __launch_bounds__(kMtWG)
per_update_kernel(double* tree, int64_t cap, int logcap, const int64_t* __restrict__ idx,
                  const double* __restrict__ leaf, const float* __restrict__ td, int64_t td_stride,
                  int n, int hbits, int64_t first_slot, int64_t memory_size, double eps,
                  double alpha) {
  extern __shared__ __align__(16) u64 s_dyn[];
  u64* table = s_dyn;
  double2* s_top = reinterpret_cast<double2*>(s_dyn);
  double* scr = reinterpret_cast<double*>(reinterpret_cast<char*>(s_dyn) + per_update_main(hbits));
  double2* nodes = reinterpret_cast<double2*>(tree);
  const int tid = threadIdx.x;
  const int glevels = logcap > 10 ? logcap - 10 : logcap;
  const double maxp = tree[0];
  int slot[kPerE];
  double lv[kPerE];
  bool live[kPerE];
  double pmax = 0.0;
#pragma unroll
  for (int k = 0; k < kPerE; ++k) {
    const int e = tid + k * kMtWG;
    live[k] = e < n;
    slot[k] = 0;
    lv[k] = 0.0;
    if (live[k]) {
      if constexpr (MODE == PER_SET) {
        slot[k] = (int)idx[e];
        lv[k] = leaf[e];
      } else if constexpr (MODE == PER_INSERT) {
        slot[k] = (int)((first_slot + e) % memory_size);
        lv[k] = pow(maxp, alpha);
      } else {
        slot[k] = (int)idx[e];
        const double p = fabs((double)td[(int64_t)e * td_stride]) + eps;
        pmax = fmax(pmax, p);
        lv[k] = pow(p, alpha);
      }
    }
  }
  if constexpr (MODE != PER_INSERT) {
    const int cells = 1 << hbits, mask = cells - 1;
    for (int i = tid; i < cells; i += kMtWG) table[i] = 0;
    __syncthreads();
    // every probe loop is bounded by the table size (the table is never more
    // than half full, so an empty or matching cell comes long before that)
#pragma unroll
    for (int k = 0; k < kPerE; ++k)
      if (live[k]) {
        const u64 key = (u64)slot[k] + 1, mine = (key << 13) | (u64)(tid + k * kMtWG);
        int h = (int)(((uint32_t)slot[k] * 2654435761U) >> (32 - hbits));
        for (int p = 0; p < cells; ++p) {
          const u64 old = atomicCAS(&table[h], (u64)0, mine);
          if (old == 0) break;
          if ((old >> 13) == key) { atomicMax(&table[h], mine); break; }
          h = (h + 1) & mask;
        }
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPerE; ++k)
      if (live[k]) {
        const u64 key = (u64)slot[k] + 1, mine = (key << 13) | (u64)(tid + k * kMtWG);
        int h = (int)(((uint32_t)slot[k] * 2654435761U) >> (32 - hbits));
        bool last = false;
        for (int p = 0; p < cells; ++p) {
          const u64 cur = table[h];
          if ((cur >> 13) == key) { last = cur == mine; break; }
          h = (h + 1) & mask;
        }
        live[k] = last;
      }
  }
#pragma unroll
  for (int k = 0; k < kPerE; ++k)
    if (live[k]) nodes[cap + slot[k]] = make_double2(lv[k], lv[k]);
  for (int level = 1; level <= glevels; ++level) {
    __syncthreads();
    double2 l[kPerE], r[kPerE];
#pragma unroll
    for (int k = 0; k < kPerE; ++k)
      if (live[k]) {
        const int64_t node = (cap + slot[k]) >> level;
        l[k] = nodes[2 * node];
        r[k] = nodes[2 * node + 1];
      }
#pragma unroll
    for (int k = 0; k < kPerE; ++k)
      if (live[k]) {
        const int64_t node = (cap + slot[k]) >> level;
        nodes[node] = make_double2(l[k].x + r[k].x, r[k].y < l[k].y ? r[k].y : l[k].y);
      }
  }
  if (logcap > 10) {
    __syncthreads();                       // the level is complete; the table is done with
    s_top[kMtWG + tid] = nodes[kMtWG + tid];
    for (int wdt = kMtWG / 2; wdt >= 1; wdt >>= 1) {
      __syncthreads();
      if (tid < wdt) {
        const double2 a = s_top[2 * (wdt + tid)], b = s_top[2 * (wdt + tid) + 1];
        s_top[wdt + tid] = make_double2(a.x + b.x, b.y < a.y ? b.y : a.y);
      }
    }
    __syncthreads();
    if (tid) nodes[tid] = s_top[tid];
  }
  if constexpr (MODE == PER_TD) {
    pmax = block_max_d(pmax, scr);
    if (tid == 0) tree[0] = fmax(maxp, pmax);
  }
}

// cells of the last-occurrence table: a power of two >= 2n, at least 1024
static int per_hbits(int n) {
  int b = 10;
  while ((1 << b) < 2 * n) ++b;
  return b;
}

template <int MODE>
static int launch_per_update(const char* what, double* tree, int64_t cap, const int64_t* idx,
                             const double* leaf, const float* td, int64_t td_stride, int n,
                             int64_t first_slot, int64_t memory_size, double eps, double alpha,
                             hipStream_t s) {
  int lc = 0;
  while (((int64_t)1 << lc) < cap) ++lc;
  const int hbits = MODE == PER_INSERT ? 0 : per_hbits(n);
  const size_t lds = per_update_lds(hbits);
  allow_lds(per_update_kernel<MODE>, lds);
  hipLaunchKernelGGL(per_update_kernel<MODE>, dim3(1), dim3(kMtWG), lds, s, tree, cap, lc, idx, leaf,
                     td, td_stride, n, hbits, first_slot, memory_size, eps, alpha);
  return check_launch(what);
}

int launch_per_set(double* tree, int64_t cap, const int64_t* idx, const double* leaf, int64_t n,
                   hipStream_t s) {
  for (int64_t o = 0; o < n; o += kPerUpd) {       // in order: a later launch overwrites
    const int m = (int)(n - o < kPerUpd ? n - o : kPerUpd);
    RC_CHECK(launch_per_update<PER_SET>("per_update_kernel<set>", tree, cap, idx + o, leaf + o,
                                        nullptr, 0, m, 0, 1, 0.0, 0.0, s));
  }
  return SMI_OK;
}

int launch_per_insert(double* tree, int64_t cap, int64_t first_slot, int64_t n, int64_t memory_size,
                      double alpha, hipStream_t s) {
  // n > memory_size: only the last memory_size rows survive, one leaf each
  const int64_t cnt = n < memory_size ? n : memory_size;
  const int64_t start = (first_slot + (n - cnt)) % memory_size;
  for (int64_t o = 0; o < cnt; o += kPerUpd) {
    const int m = (int)(cnt - o < kPerUpd ? cnt - o : kPerUpd);
    RC_CHECK(launch_per_update<PER_INSERT>("per_update_kernel<insert>", tree, cap, nullptr, nullptr,
                                           nullptr, 0, m, (start + o) % memory_size, memory_size,
                                           0.0, alpha, s));
  }
  return SMI_OK;
}

int launch_per_update_td(double* tree, int64_t cap, const int64_t* idx, const float* td,
                         int64_t td_stride, int64_t n, double eps, double alpha, hipStream_t s) {
  for (int64_t o = 0; o < n; o += kPerUpd) {
    const int m = (int)(n - o < kPerUpd ? n - o : kPerUpd);
    RC_CHECK(launch_per_update<PER_TD>("per_update_kernel<td>", tree, cap, idx + o, nullptr,
                                       td + o * td_stride, td_stride, m, 0, 1, eps, alpha, s));
  }
  return SMI_OK;
}

// One workgroup of kMtWG threads.  The 2 * batch tempered words are produced
// in stream order into LDS, kPerChunk draws at a time, across as many twists
// as that takes (a draw may take its first word before a twist and its second
// after it); then every thread pairs the words of its draws into 53-bit
// doubles, descends and writes idx and w.  The top kPerTop nodes of the sum
// tree are read once into LDS (the first 11 levels of each descent), the rest
// comes from L2.  The advanced state goes back exactly as after 2 * batch
// genrand_uint32 calls (a twist happens only when a word is needed).
__global__ void __launch_bounds__(kMtWG)
per_sample_kernel(const double* __restrict__ tree, int64_t cap, int64_t len,
                  uint32_t* __restrict__ st, int64_t batch, double beta,
                  int64_t* __restrict__ idx_out, float* __restrict__ w_out) {
  __shared__ uint32_t mt[kMtN];
  __shared__ uint32_t words[2 * kPerChunk];
  __shared__ double top[kPerTop];
  __shared__ double s_term[64];
  __shared__ double s_total, s_maxw;
  __shared__ int s_pos;
  const int tid = threadIdx.x;
  for (int i = tid; i < kMtN; i += kMtWG) mt[i] = st[i];
  if (tid == 0) s_pos = (int)st[kMtN];
  const int ntop = (int)(2 * cap < kPerTop ? 2 * cap : kPerTop);
  for (int i = tid; i < ntop; i += kMtWG) top[i] = i ? tree[2 * (int64_t)i] : 0.0;
  // the terms of total, one lane each (one round trip): lane 0 the node whose
  // range ends at leaf len-2, lane l the left sibling of that node's ancestor-
  // or-self l-1 levels up where it is a right child
  const int64_t stop = per_reduce_stop(cap, len - 2);
  if (tid < 64) {
    double t = -1.0;                                  // no term (tree sums are >= 0)
    if (tid == 0) t = tree[2 * stop];
    else {
      const int64_t a = stop >> (tid - 1);
      if (a > 1 && (a & 1)) t = tree[2 * (a - 1)];
    }
    s_term[tid] = t;
  }
  __syncthreads();
  if (tid == 0) {
    double acc = s_term[0];
    for (int l = 1; l < 64; ++l)
      if ((stop >> (l - 1)) > 1 && ((stop >> (l - 1)) & 1)) acc = s_term[l] + acc;
    s_total = acc;
    const double p_min = tree[3] / tree[2];
    s_maxw = pow(p_min * (double)len, -beta);
  }
  __syncthreads();
  const double total = s_total, max_w = s_maxw, sum = tree[2];
  for (int64_t done = 0; done < batch; done += kPerChunk) {
    const int nd = (int)(batch - done < kPerChunk ? batch - done : kPerChunk);
    const int nw = 2 * nd;
    int filled = 0;
    while (filled < nw) {
      if (s_pos >= kMtN) {
        mt_twist_wg(mt, tid);
        if (tid == 0) s_pos = 0;
        __syncthreads();
      }
      const int pos = s_pos;
      const int take = kMtN - pos < nw - filled ? kMtN - pos : nw - filled;
      if (tid < take) words[filled + tid] = mt_temper(mt[pos + tid]);
      __syncthreads();
      if (tid == 0) s_pos = pos + take;
      filled += take;
      __syncthreads();
    }
    for (int d = tid; d < nd; d += kMtWG) {
      double mass = per_u53(words[2 * d], words[2 * d + 1]) * total;
      int64_t i = 1;
      while (i < cap) {
        const int64_t c = 2 * i;
        const double s = c < ntop ? top[c] : tree[2 * c];
        if (s > mass) i = c;
        else { mass -= s; i = c + 1; }
      }
      int64_t slot = i - cap;
      if (slot > len - 1) slot = len - 1;
      idx_out[done + d] = slot;
      w_out[done + d] = per_weight(tree[2 * (cap + slot)], sum, max_w, len, beta);
    }
    __syncthreads();                                  // words are overwritten by the next pass
  }
  for (int i = tid; i < kMtN; i += kMtWG) st[i] = mt[i];
  if (tid == 0) st[kMtN] = (uint32_t)s_pos;
}

int launch_per_sample(const double* tree, int64_t cap, int64_t len, uint32_t* st, int64_t batch,
                      double beta, int64_t* idx_out, float* w_out, hipStream_t s) {
  hipLaunchKernelGGL(per_sample_kernel, dim3(1), dim3(kMtWG), 0, s, tree, cap, len, st, batch, beta,
                     idx_out, w_out);
  return check_launch("per_sample_kernel");
}

}  // namespace smi
