// sampler_kernels.hip — CPython-exact uniform replay index sampling and the
// replay row gather (UniformReplay.sample, surreal/replay/uniform_replay.py:43-47),
// and the pixel replay's fused frame + row gather (UniformReplay.sample_batch),
// with the gather and the insert scatter of its frame-shared store.
//
// The reference draws [random.randint(0, n-1) for _ in range(B)] from the
// Python stdlib generator: MT19937 (Matsumoto & Nishimura 1998) seeded by
// init_by_array with the 32-bit little-endian limbs of |seed|, and
// randint -> randrange -> _randbelow(n): k = n.bit_length(),
// r = genrand_uint32() >> (32 - k), rejected while r >= n (k <= 32 here, so one
// 32-bit word per attempt).  State: 624 words + position (625 uint32).
//
// Device algorithm (one workgroup of 1024 threads): the 624-word twist is done
// in its three dependency phases ([0,227) from old words, [227,454) and
// [454,623) from freshly twisted words 227 back, then word 623); tempering and
// the accept test are per-word parallel; a block prefix sum over accept flags
// places the accepted draws in stream order, so the output is the same
// sequence CPython produces, and exactly as many words are consumed.
#include "smi_device.hpp"
#include "smi_internal.hpp"
#include "mt19937.hpp"

namespace smi {

// ------------------------------------------------------------------ host
static void mt_init_genrand(uint32_t* mt, uint32_t s) {
  mt[0] = s;
  for (int i = 1; i < kMtN; ++i) mt[i] = 1812433253U * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
}

void mt_seed_host(uint64_t seed, uint32_t* st) {
  uint32_t key[2];
  int klen;
  key[0] = (uint32_t)(seed & 0xffffffffULL);
  key[1] = (uint32_t)(seed >> 32);
  klen = key[1] ? 2 : 1;
  uint32_t* mt = st;
  mt_init_genrand(mt, 19650218U);
  int i = 1, j = 0;
  for (int k = (kMtN > klen ? kMtN : klen); k; --k) {
    mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525U)) + key[j] + (uint32_t)j;
    ++i; ++j;
    if (i >= kMtN) { mt[0] = mt[kMtN - 1]; i = 1; }
    if (j >= klen) j = 0;
  }
  for (int k = kMtN - 1; k; --k) {
    mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941U)) - (uint32_t)i;
    ++i;
    if (i >= kMtN) { mt[0] = mt[kMtN - 1]; i = 1; }
  }
  mt[0] = 0x80000000U;
  st[kMtN] = kMtN;  // position: next call twists
}

uint32_t mt_next_host(uint32_t* st) {
  uint32_t* mt = st;
  if (st[kMtN] >= (uint32_t)kMtN) {
    int kk = 0;
    for (; kk < kMtN - kMtM; ++kk) mt[kk] = mt_mix(mt[kk], mt[kk + 1], mt[kk + kMtM]);
    for (; kk < kMtN - 1; ++kk) mt[kk] = mt_mix(mt[kk], mt[kk + 1], mt[kk + (kMtM - kMtN)]);
    mt[kMtN - 1] = mt_mix(mt[kMtN - 1], mt[0], mt[kMtM - 1]);
    st[kMtN] = 0;
  }
  return mt_temper(mt[st[kMtN]++]);
}

static int bit_length(uint64_t n) {
  int k = 0;
  while (n) { ++k; n >>= 1; }
  return k;
}

int mt_randint_host(uint32_t* st, int64_t n, int64_t batch, int64_t* out) {
  const int k = bit_length((uint64_t)n);
  for (int64_t b = 0; b < batch; ++b) {
    uint32_t r;
    do { r = mt_next_host(st) >> (32 - k); } while ((int64_t)r >= n);
    out[b] = (int64_t)r;
  }
  return SMI_OK;
}

// ---------------------------------------------------------------- device
__global__ void __launch_bounds__(kMtWG)
mt_randint_kernel(uint32_t* __restrict__ st, int64_t n, int k, int64_t batch,
                  int64_t* __restrict__ out) {
  __shared__ uint32_t mt[kMtN];
  __shared__ int wsum[kMtWG / 64];
  __shared__ int s_pos;
  const int tid = threadIdx.x;
  for (int i = tid; i < kMtN; i += kMtWG) mt[i] = st[i];
  if (tid == 0) s_pos = (int)st[kMtN];
  __syncthreads();
  int64_t filled = 0;
  while (filled < batch) {
    if (s_pos >= kMtN) {
      mt_twist_wg(mt, tid);
      if (tid == 0) s_pos = 0;
      __syncthreads();
    }
    const int pos = s_pos;
    const int avail = kMtN - pos;
    // accept test per word in stream order
    int acc = 0;
    int64_t r = 0;
    if (tid < avail) {
      r = (int64_t)(mt_temper(mt[pos + tid]) >> (32 - k));
      acc = r < n ? 1 : 0;
    }
    // block exclusive scan of acc
    const int lane = tid & 63, wave = tid >> 6;
    const unsigned long long bal = __ballot(acc);
    const int wpre = __popcll(bal & ((1ULL << lane) - 1ULL));
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kMtWG / 64; ++w) {
      if (w < wave) before += wsum[w];
      total += wsum[w];
    }
    const int rank = before + wpre;
    const int64_t need = batch - filled;
    if (acc && rank < need) out[filled + rank] = r;
    // words consumed: all available, or up to the word giving the need-th draw
    __syncthreads();
    if (total >= need) {
      if (acc && rank == need - 1) s_pos = pos + tid + 1;
      __syncthreads();
      filled = batch;
    } else {
      if (tid == 0) s_pos = kMtN;
      __syncthreads();
      filled += total;
    }
    __syncthreads();
  }
  for (int i = tid; i < kMtN; i += kMtWG) st[i] = mt[i];
  if (tid == 0) st[kMtN] = (uint32_t)s_pos;
}

int launch_mt_randint(uint32_t* st, int64_t n, int64_t batch, int64_t* out, hipStream_t s) {
  if (n < 1 || n > 0xffffffffLL) return set_error(SMI_E_ARG, "mt_randint: n must be in [1, 2^32]");
  if (batch <= 0) return SMI_OK;
  const int k = bit_length((uint64_t)n);
  hipLaunchKernelGGL(mt_randint_kernel, dim3(1), dim3(kMtWG), 0, s, st, n, k, batch, out);
  return check_launch("mt_randint_kernel");
}

// ------------------------------------------------------------ row gather
// out[i][:] = table[idx[i]][:].  Output-ordered (coalesced stores); 16-byte
// elements when rows are float4-aligned, 32-bit index arithmetic when the
// output fits (a 64-bit divide per element costs more than the load), and four
// independent loads in flight per thread.
template <typename V, typename I>
__device__ __forceinline__ void gather_body(const V* __restrict__ table, I cols,
                                            const int64_t* __restrict__ idx, I total,
                                            V* __restrict__ out) {
  const I stride = (I)gridDim.x * kWG;
  I e = (I)blockIdx.x * kWG + threadIdx.x;
  for (; e + 3 * stride < total; e += 4 * stride) {
    V v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const I f = e + u * stride;
      const I i = f / cols, c = f - i * cols;
      v[u] = table[idx[i] * (int64_t)cols + c];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) out[e + u * stride] = v[u];
  }
  for (; e < total; e += stride) {
    const I i = e / cols, c = e - i * cols;
    out[e] = table[idx[i] * (int64_t)cols + c];
  }
}

__global__ void __launch_bounds__(kWG)
gather_rows_kernel(const float* __restrict__ table, int64_t cols, const int64_t* __restrict__ idx,
                   int64_t batch, float* __restrict__ out) {
  const uintptr_t al = reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out);
  const bool v4 = (cols & 3) == 0 && (al & 15) == 0;
  // even widths (the DDPG row [s | a | r | s' | d] of HalfCheetah is 42 floats)
  // move as 8-byte elements
  const bool v2 = !v4 && (cols & 1) == 0 && (al & 7) == 0;
  const int64_t c = v4 ? cols >> 2 : v2 ? cols >> 1 : cols;
  const int64_t total = batch * c;
  if (total < ((int64_t)1 << 31)) {
    if (v4) gather_body<float4, uint32_t>(reinterpret_cast<const float4*>(table), (uint32_t)c, idx,
                                          (uint32_t)total, reinterpret_cast<float4*>(out));
    else if (v2) gather_body<float2, uint32_t>(reinterpret_cast<const float2*>(table), (uint32_t)c,
                                               idx, (uint32_t)total, reinterpret_cast<float2*>(out));
    else gather_body<float, uint32_t>(table, (uint32_t)c, idx, (uint32_t)total, out);
  } else {
    if (v4) gather_body<float4, int64_t>(reinterpret_cast<const float4*>(table), c, idx, total,
                                         reinterpret_cast<float4*>(out));
    else if (v2) gather_body<float2, int64_t>(reinterpret_cast<const float2*>(table), c, idx, total,
                                              reinterpret_cast<float2*>(out));
    else gather_body<float, int64_t>(table, c, idx, total, out);
  }
}

int launch_gather_rows(const float* table, int64_t cols, const int64_t* idx, int64_t batch,
                       float* out, hipStream_t s) {
  const int64_t work = batch * ((cols & 3) == 0 ? cols / 4 : (cols & 1) == 0 ? cols / 2 : cols);
  if (work <= 0) return SMI_OK;
  int64_t g = (work + kWG - 1) / kWG;
  g = (g + 3) / 4;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((int)g), dim3(kWG), 0, s, table, cols, idx, batch, out);
  return check_launch("gather_rows_kernel");
}

// ------------------------------------------------- replay gather (frames)
// Pixel replay sample: pix_out[i] = frames[idx[i]], pix_next_out[i] =
// frames_next[idx[i]] (uint8 frames of frame_bytes each) and, when a table is
// given, rows_out[i] = table[idx[i]], in one launch.
//
// A work item is (sample, side, chunk): one workgroup moves one 16 KiB chunk
// (kRgU 16-byte vectors per lane) of one frame, so idx[i] and both base
// addresses are workgroup-uniform (scalar loads and arithmetic), every lane
// issues its kRgU loads before its first store (32 waves per CU x 4 KiB = 128
// KiB in flight per CU), and source offsets are 64-bit (the reference ring,
// 333,333 x 63,504 B, is 21 GB per side).  Items are dealt to a capped 1-D
// grid.  The float side rows follow in the same launch through gather_body.
//
// Plain loads and stores (B = 512 of 9 x 84 x 84, one MI355X: plain 25.8-26.0
// us, nontemporal loads 26.3, stores 28.5, both 27.7): the
// frames are read by the conv forward right after this launch.
constexpr int kRgU = 4;
constexpr int kRgChunk = kWG * kRgU;   // 16-byte vectors (VEC) or bytes x 16 per work item
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void gather_rows_side(const float* __restrict__ table, int64_t cols,
                                                 const int64_t* __restrict__ idx, int64_t batch,
                                                 float* __restrict__ out) {
  // element width and index width chosen as gather_rows_kernel chooses them
  const uintptr_t al = reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out);
  const bool v4 = (cols & 3) == 0 && (al & 15) == 0;
  const bool v2 = !v4 && (cols & 1) == 0 && (al & 7) == 0;
  const int64_t c = v4 ? cols >> 2 : v2 ? cols >> 1 : cols;
  const int64_t total = batch * c;
  if (total < ((int64_t)1 << 31)) {
    if (v4) gather_body<float4, uint32_t>(reinterpret_cast<const float4*>(table), (uint32_t)c, idx,
                                          (uint32_t)total, reinterpret_cast<float4*>(out));
    else if (v2) gather_body<float2, uint32_t>(reinterpret_cast<const float2*>(table), (uint32_t)c,
                                               idx, (uint32_t)total, reinterpret_cast<float2*>(out));
    else gather_body<float, uint32_t>(table, (uint32_t)c, idx, (uint32_t)total, out);
  } else {
    if (v4) gather_body<float4, int64_t>(reinterpret_cast<const float4*>(table), c, idx, total,
                                         reinterpret_cast<float4*>(out));
    else if (v2) gather_body<float2, int64_t>(reinterpret_cast<const float2*>(table), c, idx, total,
                                              reinterpret_cast<float2*>(out));
    else gather_body<float, int64_t>(table, c, idx, total, out);
  }
}

// VEC: frame_bytes % 16 == 0 and all four pixel pointers 16-byte aligned;
// otherwise bytes (correct for any size and alignment; no learner-valid frame
// takes it, cnn_check demands C*H*W % 16 == 0).  cpf = chunks per frame.
template <bool VEC>
__global__ void __launch_bounds__(kWG)
replay_gather_kernel(const float* __restrict__ table, int64_t cols,
                     const uint8_t* __restrict__ frames, const uint8_t* __restrict__ frames_next,
                     int64_t frame_bytes, const int64_t* __restrict__ idx, int64_t batch,
                     float* __restrict__ rows_out, uint8_t* __restrict__ pix_out,
                     uint8_t* __restrict__ pix_next_out, int64_t cpf) {
  const int64_t items = batch * 2 * cpf;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t s = it / cpf, chunk = it - s * cpf;
    const int64_t i = s >> 1;
    const bool nxt = (s & 1) != 0;
    const uint8_t* src = (nxt ? frames_next : frames) + idx[i] * frame_bytes;
    uint8_t* dst = (nxt ? pix_next_out : pix_out) + i * frame_bytes;
    if constexpr (VEC) {
      const u32x4* s4 = reinterpret_cast<const u32x4*>(src);
      u32x4* d4 = reinterpret_cast<u32x4*>(dst);
      // frame_bytes < 2^31 (checked by the entry point): in-frame offsets are int.
      // Tail lanes load the frame's last vector (in bounds, unconditional, so
      // the kRgU loads issue back to back) and skip the store.
      const int nvec = (int)(frame_bytes >> 4);
      const int v0 = (int)chunk * kRgChunk + (int)threadIdx.x;
      u32x4 v[kRgU];
#pragma unroll
      for (int u = 0; u < kRgU; ++u) {
        const int e = min(v0 + u * kWG, nvec - 1);
        v[u] = s4[e];
      }
#pragma unroll
      for (int u = 0; u < kRgU; ++u) {
        const int e = v0 + u * kWG;
        if (e < nvec) d4[e] = v[u];
      }
    } else {
      const int64_t b0 = chunk * kRgChunk * 16;
      const int64_t b1 = b0 + kRgChunk * 16 < frame_bytes ? b0 + kRgChunk * 16 : frame_bytes;
      for (int64_t b = b0 + threadIdx.x; b < b1; b += kWG) dst[b] = src[b];
    }
  }
  if (cols > 0) gather_rows_side(table, cols, idx, batch, rows_out);
}

int launch_replay_gather(const float* table, int64_t cols, const uint8_t* frames,
                         const uint8_t* frames_next, int64_t frame_bytes, const int64_t* idx,
                         int64_t batch, float* rows_out, uint8_t* pix_out, uint8_t* pix_next_out,
                         hipStream_t s) {
  if (batch <= 0) return SMI_OK;
  const uintptr_t al = reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(frames_next) |
                       reinterpret_cast<uintptr_t>(pix_out) | reinterpret_cast<uintptr_t>(pix_next_out);
  const bool vec = (frame_bytes & 15) == 0 && (al & 15) == 0;
  const int64_t cpf = (frame_bytes + kRgChunk * 16 - 1) / (kRgChunk * 16);
  int64_t g = batch * 2 * cpf;
  if (g > 4096) g = 4096;
  if (vec)
    hipLaunchKernelGGL(replay_gather_kernel<true>, dim3((int)g), dim3(kWG), 0, s, table, cols, frames,
                       frames_next, frame_bytes, idx, batch, rows_out, pix_out, pix_next_out, cpf);
  else
    hipLaunchKernelGGL(replay_gather_kernel<false>, dim3((int)g), dim3(kWG), 0, s, table, cols,
                       frames, frames_next, frame_bytes, idx, batch, rows_out, pix_out,
                       pix_next_out, cpf);
  return check_launch("replay_gather_kernel");
}

// ------------------------------------- replay gather (frame-shared store)
// The frame-shared pixel replay keeps every (C/S, H, W) frame once in `store`
// and names the S frames of each observation in fid[slot][side][k].  The
// sample is the same output as replay_gather_kernel: pix_out[i] = the S frames
// fid[idx[i]][0][:] one after the other, pix_next_out[i] from side 1.
//
// A work item is (sample, side, chunk) of the DESTINATION side (S * fbytes
// bytes), chunked as above, so the chunks stay full where a 21,168-byte frame
// alone would leave every second one 29 % full.  idx[i], the S ids of the side
// (one dependent load of 4 S bytes) and the S source offsets are workgroup-
// uniform; a lane picks its source frame from its destination vector index
// (compares against multiples of the vectors per frame, no divide) and frame
// boundaries fall on vector boundaries because fbytes % 16 == 0.  Every lane
// issues its kRgU loads before its first store; tail lanes re-read the side's
// last vector and skip the store.  Source offsets are 64-bit (the reference
// store, 416,666 x 21,168 B, is 8.8 GB).
constexpr int kRgMaxStack = 4;

// STACK = S is a template parameter: the S ids of a side are one block of
// scalar loads and a lane's source frame is picked by S - 1 selects, no branch.
template <bool VEC, int STACK>
__global__ void __launch_bounds__(kWG)
replay_gather_shared_kernel(const float* __restrict__ table, int64_t cols,
                            const uint8_t* __restrict__ store, const int32_t* __restrict__ fid,
                            int64_t fbytes, const int64_t* __restrict__ idx, int64_t batch,
                            float* __restrict__ rows_out, uint8_t* __restrict__ pix_out,
                            uint8_t* __restrict__ pix_next_out, int64_t cps) {
  const int64_t items = batch * 2 * cps;
  const int64_t side_bytes = STACK * fbytes;            // < 2^31 (checked by the entry point)
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t s = it / cps, chunk = it - s * cps;
    const int64_t i = s >> 1;
    const bool nxt = (s & 1) != 0;
    const int32_t* ids = fid + (idx[i] * 2 + (nxt ? 1 : 0)) * STACK;
    int64_t off[STACK];                                  // byte offset of frame k in the store
#pragma unroll
    for (int k = 0; k < STACK; ++k) off[k] = (int64_t)ids[k] * fbytes;
    uint8_t* dst = (nxt ? pix_next_out : pix_out) + i * side_bytes;
    if constexpr (VEC) {
      u32x4* d4 = reinterpret_cast<u32x4*>(dst);
      const int nvf = (int)(fbytes >> 4);          // vectors per frame
      const int nvec = STACK * nvf;                // vectors per side
      const int v0 = (int)chunk * kRgChunk + (int)threadIdx.x;
      u32x4 v[kRgU];
#pragma unroll
      for (int u = 0; u < kRgU; ++u) {
        // Tail lanes load the side's last vector (in bounds, unconditional) and
        // skip the store.
        const int e = min(v0 + u * kWG, nvec - 1);
        int64_t o = off[0];
        int r = e;
#pragma unroll
        for (int k = 1; k < STACK; ++k) {
          const bool past = e >= k * nvf;
          o = past ? off[k] : o;
          r = past ? e - k * nvf : r;
        }
        v[u] = *reinterpret_cast<const u32x4*>(store + o + ((int64_t)r << 4));
      }
#pragma unroll
      for (int u = 0; u < kRgU; ++u) {
        const int e = v0 + u * kWG;
        if (e < nvec) d4[e] = v[u];
      }
    } else {
      const int64_t b0 = chunk * kRgChunk * 16;
      const int64_t b1 = b0 + kRgChunk * 16 < side_bytes ? b0 + kRgChunk * 16 : side_bytes;
      for (int64_t b = b0 + threadIdx.x; b < b1; b += kWG) {
        int64_t o = off[0], r = b;
#pragma unroll
        for (int k = 1; k < STACK; ++k) {
          const bool past = b >= k * fbytes;
          o = past ? off[k] : o;
          r = past ? b - k * fbytes : r;
        }
        dst[b] = store[o + r];
      }
    }
  }
  if (cols > 0) gather_rows_side(table, cols, idx, batch, rows_out);
}

template <bool VEC>
static void launch_rgs(int stack, int g, hipStream_t s, const float* table, int64_t cols,
                       const uint8_t* store, const int32_t* fid, int64_t fbytes, const int64_t* idx,
                       int64_t batch, float* rows_out, uint8_t* pix_out, uint8_t* pix_next_out,
                       int64_t cps) {
#define SMI_RGS(S) \
  hipLaunchKernelGGL((replay_gather_shared_kernel<VEC, S>), dim3(g), dim3(kWG), 0, s, table, cols, \
                     store, fid, fbytes, idx, batch, rows_out, pix_out, pix_next_out, cps)
  switch (stack) {
    case 1: SMI_RGS(1); break;
    case 2: SMI_RGS(2); break;
    case 3: SMI_RGS(3); break;
    default: SMI_RGS(4); break;
  }
#undef SMI_RGS
}

int launch_replay_gather_shared(const float* table, int64_t cols, const uint8_t* store,
                                const int32_t* fid, int stack, int64_t fbytes, const int64_t* idx,
                                int64_t batch, float* rows_out, uint8_t* pix_out,
                                uint8_t* pix_next_out, hipStream_t s) {
  if (batch <= 0) return SMI_OK;
  if (stack < 1 || stack > kRgMaxStack)
    return set_error(SMI_E_ARG, "replay_gather_shared: stack outside [1, 4]");
  const uintptr_t al = reinterpret_cast<uintptr_t>(store) | reinterpret_cast<uintptr_t>(pix_out) |
                       reinterpret_cast<uintptr_t>(pix_next_out);
  const bool vec = (fbytes & 15) == 0 && (al & 15) == 0;
  const int64_t side_bytes = (int64_t)stack * fbytes;
  const int64_t cps = (side_bytes + kRgChunk * 16 - 1) / (kRgChunk * 16);
  int64_t g = batch * 2 * cps;
  if (g > 4096) g = 4096;
  if (vec)
    launch_rgs<true>(stack, (int)g, s, table, cols, store, fid, fbytes, idx, batch, rows_out, pix_out,
                     pix_next_out, cps);
  else
    launch_rgs<false>(stack, (int)g, s, table, cols, store, fid, fbytes, idx, batch, rows_out,
                      pix_out, pix_next_out, cps);
  return check_launch("replay_gather_shared_kernel");
}

// ------------------------------------- replay insert (frame-shared store)
// One launch per insert call, reading one staged block: the m new frames go
// to store[fslots[j]] (16-byte vectors when fbytes % 16 == 0 and both frame
// pointers are aligned, bytes otherwise; no two fslots are equal, the host
// allocator hands a slot out once per call), and the last cnt = min(n,
// memory_size) of the n rows and of their [2][S] frame ids go to the ring
// slots (first_slot + e) % memory_size, e = n - cnt .. n - 1 (the wrap rule of
// launch_per_insert).  Flat grid-stride loops: the insert is bound by the
// host-to-device copy in front of it, not by this kernel.
template <bool VEC>
__global__ void __launch_bounds__(kWG)
replay_insert_shared_kernel(float* __restrict__ table, int64_t cols, int32_t* __restrict__ fid,
                            int64_t ids_per_row, uint8_t* __restrict__ store, int64_t fbytes,
                            int64_t memory_size, int64_t first_slot,
                            const float* __restrict__ rows, const int32_t* __restrict__ ids,
                            int64_t n, int64_t cnt, const uint8_t* __restrict__ frames,
                            const int32_t* __restrict__ fslots, int64_t m) {
  const int64_t stride = (int64_t)gridDim.x * kWG;
  const int64_t t0 = (int64_t)blockIdx.x * kWG + threadIdx.x;
  if constexpr (VEC) {
    const int64_t nvf = fbytes >> 4;
    const u32x4* f4 = reinterpret_cast<const u32x4*>(frames);
    for (int64_t e = t0; e < m * nvf; e += stride) {
      const int64_t j = e / nvf, r = e - j * nvf;
      reinterpret_cast<u32x4*>(store + (int64_t)fslots[j] * fbytes)[r] = f4[e];
    }
  } else {
    for (int64_t e = t0; e < m * fbytes; e += stride) {
      const int64_t j = e / fbytes, r = e - j * fbytes;
      store[(int64_t)fslots[j] * fbytes + r] = frames[e];
    }
  }
  const int64_t skip = n - cnt;
  for (int64_t e = t0; e < cnt * cols; e += stride) {
    const int64_t r = skip + e / cols, c = e % cols;
    table[((first_slot + r) % memory_size) * cols + c] = rows[r * cols + c];
  }
  for (int64_t e = t0; e < cnt * ids_per_row; e += stride) {
    const int64_t r = skip + e / ids_per_row, c = e % ids_per_row;
    fid[((first_slot + r) % memory_size) * ids_per_row + c] = ids[r * ids_per_row + c];
  }
}

int launch_replay_insert_shared(float* table, int64_t cols, int32_t* fid, int stack, uint8_t* store,
                                int64_t fbytes, int64_t memory_size, int64_t first_slot,
                                const float* rows, const int32_t* ids, int64_t n,
                                const uint8_t* frames, const int32_t* fslots, int64_t m,
                                hipStream_t s) {
  if (n <= 0 && m <= 0) return SMI_OK;
  const int64_t cnt = n < memory_size ? n : memory_size;
  const uintptr_t al = reinterpret_cast<uintptr_t>(store) | reinterpret_cast<uintptr_t>(frames);
  const bool vec = (fbytes & 15) == 0 && (al & 15) == 0;
  int64_t work = vec ? m * (fbytes >> 4) : m * fbytes;
  if (cnt * cols > work) work = cnt * cols;
  if (cnt * 2 * stack > work) work = cnt * 2 * stack;
  int64_t g = (work + kWG - 1) / kWG;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  if (vec)
    hipLaunchKernelGGL(replay_insert_shared_kernel<true>, dim3((int)g), dim3(kWG), 0, s, table, cols,
                       fid, (int64_t)2 * stack, store, fbytes, memory_size, first_slot, rows, ids, n,
                       cnt, frames, fslots, m);
  else
    hipLaunchKernelGGL(replay_insert_shared_kernel<false>, dim3((int)g), dim3(kWG), 0, s, table, cols,
                       fid, (int64_t)2 * stack, store, fbytes, memory_size, first_slot, rows, ids, n,
                       cnt, frames, fslots, m);
  return check_launch("replay_insert_shared_kernel");
}

}  // namespace smi
