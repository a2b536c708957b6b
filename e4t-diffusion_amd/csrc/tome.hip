// Token merging (ToMe, Bolya & Hoffman, "Token Merging for Stable Diffusion") around the UNet's self-attention, for gfx950.
//
// The reference lists it as its last open TODO ("Support ToMe for more efficient training", README.md:116); the call site is the
// `attn1` of BasicTransformerBlock (e4t/models/attention.py:181-332).  Three entry points:
//   e4t_tome_match    bipartite soft matching on a 2x2-cell split of the h x w grid -> a PLAN (plain int32 arrays, layout in e4t_hip.h)
//   e4t_tome_merge    y = M . x   (segment reduction over the plan's CSR; mean or sum)      forward merge / backward of unmerge
//   e4t_tome_unmerge  x = (residual +) y[map] (/ count)                                     forward unmerge / backward of merge
//
// Match = five launches, no host read, no float atomics, every reduction in a fixed order (the plan is bitwise equal run to run):
//   tome_tokens_kernel   which token of each cell is dst (choice), the src tokens in ascending token order (one block scan)
//   tome_norm_kernel     ||x_t||_2 per token: the squares of bf16 values are exact in fp32 and their fp64 sum does not depend on the order
//   tome_score_kernel    score^T[dst][src] = x^_dst . x^_src on v_mfma_f32_32x32x16_bf16 — the attention forward's S^T = K . Q^T without the
//                        softmax: A = a 32-row dst tile normalised once per workgroup into LDS, B = 32 src rows per wave normalised into
//                        registers, every lane owns ONE src column and 16 of the tile's 32 dst rows, so the running max / argmax are
//                        per-lane scalars; the ns x nd matrix never leaves the registers
//   tome_select_kernel   one workgroup per image: bitonic sort of (node_max descending, src position ascending) keys in LDS -> the r merged
//                        src; a second sort by (dst, src position) IS seg_src, seg_off is a binary search in it; one block scan numbers
//                        the unmerged rows.  Plain __syncthreads() only.
#include "common.h"
#include "../../include/e4t_hip.h"
#include <math.h>

namespace {

constexpr int TOME_MAX_T = 16384;
constexpr int SEL_THREADS = 1024;
constexpr int SEL_PER = 16;          // sort slots per thread: 16384 / 1024

struct TomeDims {
  int B, T, nd, ns, r, Tm;           // Tm = T' = T - r
};

// offsets (in ints) of the plan's fields for a batch of B images; the ABI part first, the match's own scratch behind it
struct PlanLayout {
  size_t map, row_tok, seg_off, seg_src, norm, node_max, node_idx, src_tok, dst_tok, total;
};
__host__ __device__ inline PlanLayout plan_layout(int B, int T, int r) {
  const int nd = T / 4, ns = T - nd;
  PlanLayout L;
  L.map = 0;
  L.row_tok = L.map + (size_t)B * T;
  L.seg_off = L.row_tok + (size_t)B * (T - r);
  L.seg_src = L.seg_off + (size_t)B * (nd + 1);
  L.norm = L.seg_src + (size_t)B * r;
  L.node_max = L.norm + (size_t)B * T;
  L.node_idx = L.node_max + (size_t)B * ns;
  L.src_tok = L.node_idx + (size_t)B * ns;
  L.dst_tok = L.src_tok + ns;
  L.total = L.dst_tok + nd;
  return L;
}

// exclusive prefix sum of one int per thread over a 1024-thread block; sc: 1024 ints of LDS
__device__ __forceinline__ int block_excl_scan(int v, int* sc) {
  const int tid = threadIdx.x;
  __syncthreads();
  sc[tid] = v;
  __syncthreads();
  for (int off = 1; off < SEL_THREADS; off <<= 1) {
    const int t = tid >= off ? sc[tid - off] : 0;
    __syncthreads();
    sc[tid] += t;
    __syncthreads();
  }
  return sc[tid] - v;
}

// ---- split: dst token of every cell, src tokens in ascending token order (shared by the batch) -------------------------------------
__global__ __launch_bounds__(SEL_THREADS) void tome_tokens_kernel(const int* __restrict__ choice, int h, int w, int* __restrict__ src_tok,
                                                                  int* __restrict__ dst_tok) {
  __shared__ int sc[SEL_THREADS];
  const int T = h * w, ws = w >> 1, nd = T >> 2, tid = threadIdx.x;
  for (int j = tid; j < nd; j += SEL_THREADS) {
    const int ch = choice ? (choice[j] & 3) : 0;
    dst_tok[j] = (2 * (j / ws) + (ch >> 1)) * w + 2 * (j % ws) + (ch & 1);
  }
  const int per = (T + SEL_THREADS - 1) / SEL_THREADS;
  const int t0 = min(tid * per, T), t1 = min(t0 + per, T);
  auto is_src = [&](int t) {
    const int y = t / w, x = t - y * w;
    const int ch = choice ? (choice[(y >> 1) * ws + (x >> 1)] & 3) : 0;
    return (((y & 1) << 1) | (x & 1)) != ch;
  };
  int cnt = 0;
  for (int t = t0; t < t1; ++t) cnt += is_src(t) ? 1 : 0;
  int pos = block_excl_scan(cnt, sc);
  for (int t = t0; t < t1; ++t)
    if (is_src(t)) src_tok[pos++] = t;          // pos < ns: exactly three tokens of every cell are src
}

// ---- norms: one wave per token -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tome_norm_kernel(const bf16_t* __restrict__ x, int ldx, long long rows, int d, float* __restrict__ norm) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const bf16_t* xp = x + row * ldx;
  double s = 0.0;
  for (int c = lane * 8; c < d; c += 64 * 8) {
    float f[8];
    unpack8(*(const uint4*)(xp + c), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += (double)(f[e] * f[e]);      // exact: 8-bit significands
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) norm[row] = sqrtf((float)s);
}

__device__ __forceinline__ uint4 normalize8(const uint4& v, float nrm) {
  float f[8];
  unpack8(v, f);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = f[e] / nrm;                 // x^ = bf16(x / ||x||), the division in fp32 (IEEE)
  return pack8(f);
}

// ---- scores: running row max / argmax over the dst tokens ---------------------------------------------------------------------------
union TFrag {
  bf16x8 v;
  uint4 q;
};

template <int NKS>      // k-steps of 16 held in registers per src row (d <= 16 NKS)
__global__ __launch_bounds__(256) void tome_score_kernel(const bf16_t* __restrict__ x, int ldx, int T, int nd, int ns, int d,
                                                         const float* __restrict__ norm, const int* __restrict__ src_tok,
                                                         const int* __restrict__ dst_tok, float* __restrict__ node_max, int* __restrict__ node_idx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* tile = (bf16_t*)smem;                 // [32][d + 8]: rows 16 (d/8 + 1) bytes apart, an odd count of 16-B slots
  const int lde = d + 8;
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, hi = lane >> 5;
  const bf16_t* xb = x + (size_t)b * T * ldx;
  const float* nb = norm + (size_t)b * T;
  const int i_lane = blockIdx.x * 128 + wave * 32 + col;
  const int i_ld = min(i_lane, ns - 1);         // lanes past the last src re-read it and store nothing
  TFrag sf[NKS];
  {
    const int tok = src_tok[i_ld];
    const float nrm = nb[tok];
    const bf16_t* xp = xb + (size_t)tok * ldx + hi * 8;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      if (ks * 16 < d) sf[ks].q = normalize8(*(const uint4*)(xp + ks * 16), nrm);
      else sf[ks].q = make_uint4(0, 0, 0, 0);
    }
  }
  float best = -INFINITY;
  int bidx = 0;
  const int nch = d >> 3;
  for (int j0 = 0; j0 < nd; j0 += 32) {
    __syncthreads();                            // the previous tile's fragment reads are done
    for (int it = tid; it < 32 * nch; it += 256) {
      const int row = it / nch, c = it - row * nch;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (j0 + row < nd) {
        const int tok = dst_tok[j0 + row];
        v = normalize8(*(const uint4*)(xb + (size_t)tok * ldx + c * 8), nb[tok]);
      }
      *(uint4*)(tile + row * lde + c * 8) = v;
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    const bf16_t* ap = tile + col * lde + hi * 8;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      if (ks * 16 < d) {
        TFrag a;
        a.q = *(const uint4*)(ap + ks * 16);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, sf[ks].v, acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {              // ascending dst within the lane: '>' keeps the lowest index of a tie
      const int j = j0 + (q & 3) + 8 * (q >> 2) + 4 * hi;
      if (j < nd && acc[q] > best) { best = acc[q]; bidx = j; }
    }
  }
  const float ob = __shfl_xor(best, 32, 64);
  const int oi = __shfl_xor(bidx, 32, 64);
  if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
  if (hi == 0 && i_lane < ns) {
    node_max[(size_t)b * ns + i_lane] = best;
    node_idx[(size_t)b * ns + i_lane] = bidx;
  }
}

// ---- top-r selection and the CSR ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void bitonic_sort(unsigned long long* keys, int P) {
  const int tid = threadIdx.x;
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < P; t += SEL_THREADS) {
        const int u = t ^ j;
        if (u > t) {
          const unsigned long long a = keys[t], c = keys[u];
          if ((a > c) == ((t & k) == 0)) { keys[t] = c; keys[u] = a; }
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(SEL_THREADS) void tome_select_kernel(TomeDims dm, int P, int* __restrict__ plan) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* keys = (unsigned long long*)smem;       // [P]; later int flag[ns] (4 ns <= 8 P)
  int* sc = (int*)(smem + (size_t)P * 8);                     // [1024]
  const int T = dm.T, nd = dm.nd, ns = dm.ns, r = dm.r, Tm = dm.Tm;
  const int b = blockIdx.x, tid = threadIdx.x;
  const PlanLayout L = plan_layout(dm.B, T, r);
  const float* node_max = (const float*)(plan + L.node_max) + (size_t)b * ns;
  const int* node_idx = plan + L.node_idx + (size_t)b * ns;
  const int* src_tok = plan + L.src_tok;
  const int* dst_tok = plan + L.dst_tok;
  int* map = plan + L.map + (size_t)b * T;
  int* row_tok = plan + L.row_tok + (size_t)b * Tm;
  int* seg_off = plan + L.seg_off + (size_t)b * (nd + 1);
  int* seg_src = plan + L.seg_src + (size_t)b * r;

  // 1. ascending sort of (~ordered(node_max), src position): the first r are the merged src, ties to the lower position
  for (int t = tid; t < P; t += SEL_THREADS) {
    unsigned long long key = ~0ull;
    if (t < ns) {
      const unsigned u = __float_as_uint(node_max[t]);
      const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
      key = ((unsigned long long)(~ord) << 32) | (unsigned)t;
    }
    keys[t] = key;
  }
  __syncthreads();
  bitonic_sort(keys, P);
  // 2. ascending sort of (dst, src position) over the merged src: the CSR's payload in its final order
  int mi[SEL_PER], mj[SEL_PER];
#pragma unroll
  for (int k = 0; k < SEL_PER; ++k) {
    const int t = tid + k * SEL_THREADS;
    mi[k] = t < r ? min((int)(unsigned)keys[t], ns - 1) : -1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SEL_PER; ++k) {
    const int t = tid + k * SEL_THREADS;
    if (t < P) keys[t] = mi[k] >= 0 ? (((unsigned long long)(unsigned)node_idx[mi[k]] << 32) | (unsigned)mi[k]) : ~0ull;
  }
  __syncthreads();
  bitonic_sort(keys, P);
#pragma unroll
  for (int k = 0; k < SEL_PER; ++k) {
    const int t = tid + k * SEL_THREADS;
    mi[k] = mj[k] = -1;
    if (t < r) {
      mi[k] = min((int)(unsigned)keys[t], ns - 1);
      mj[k] = min((int)(keys[t] >> 32), nd - 1);
      seg_src[t] = src_tok[mi[k]];
    }
  }
  for (int j = tid; j <= nd; j += SEL_THREADS) {                // seg_off[j] = first sorted entry whose dst is >= j
    const unsigned long long want = (unsigned long long)j << 32;
    int lo = 0, hi = r;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] < want) lo = mid + 1; else hi = mid;
    }
    seg_off[j] = lo;
  }
  __syncthreads();
  // 3. map / row_tok: dst rows, merged src, then the unmerged src numbered in ascending position
  int* flag = (int*)smem;
  for (int t = tid; t < ns; t += SEL_THREADS) flag[t] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SEL_PER; ++k)
    if (mi[k] >= 0) { flag[mi[k]] = 1; map[src_tok[mi[k]]] = mj[k]; }
  for (int j = tid; j < nd; j += SEL_THREADS) { const int tok = dst_tok[j]; map[tok] = j; row_tok[j] = tok; }
  __syncthreads();
  const int per = (ns + SEL_THREADS - 1) / SEL_THREADS;
  const int i0 = min(tid * per, ns), i1 = min(i0 + per, ns);
  int cnt = 0;
  for (int i = i0; i < i1; ++i) cnt += 1 - flag[i];
  int row = nd + block_excl_scan(cnt, sc);
  for (int i = i0; i < i1; ++i)
    if (!flag[i]) {
      const int tok = src_tok[i];
      if (row < Tm) { map[tok] = row; row_tok[row] = tok; }    // (always: ns - r unmerged src fill rows nd .. T' - 1)
      ++row;
    }
}

// ---- merge: y[row] = (x[dst] + sum x[seg_src]) (/ count) for row < nd, a copy of x[row_tok[row]] behind ------------------------------
__global__ __launch_bounds__(256) void tome_merge_kernel(const bf16_t* __restrict__ x, int ldx, const int* __restrict__ plan, bf16_t* __restrict__ y,
                                                         int ldy, TomeDims dm, int d, int mean) {
  const int nch = d >> 3;
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)dm.B * dm.Tm * nch) return;
  const int c = (int)(item % nch);
  const long long brow = item / nch;
  const int b = (int)(brow / dm.Tm), row = (int)(brow - (long long)b * dm.Tm);
  const PlanLayout L = plan_layout(dm.B, dm.T, dm.r);
  const bf16_t* xb = x + (size_t)b * dm.T * ldx + c * 8;
  const int tok = min(max(plan[L.row_tok + (size_t)b * dm.Tm + row], 0), dm.T - 1);
  uint4 v = *(const uint4*)(xb + (size_t)tok * ldx);
  if (row < dm.nd) {
    const int* so = plan + L.seg_off + (size_t)b * (dm.nd + 1) + row;
    const int s0 = min(max(so[0], 0), dm.r), s1 = min(max(so[1], s0), dm.r);
    if (s1 > s0) {
      float acc[8], f[8];
      unpack8(v, acc);
      const int* ss = plan + L.seg_src + (size_t)b * dm.r;
      for (int s = s0; s < s1; ++s) {
        const int st = min(max(ss[s], 0), dm.T - 1);
        unpack8(*(const uint4*)(xb + (size_t)st * ldx), f);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += f[e];
      }
      if (mean) {
        const float cntf = (float)(1 + s1 - s0);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = acc[e] / cntf;
      }
      v = pack8(acc);
    }
  }
  *(uint4*)(y + ((size_t)b * dm.Tm + row) * ldy + c * 8) = v;
}

// ---- unmerge: x_out[i] = (residual[i] +) y[map[i]] (/ count[map[i]]) -------------------------------------------------------------------
__global__ __launch_bounds__(256) void tome_unmerge_kernel(const bf16_t* __restrict__ y, int ldy, const int* __restrict__ plan,
                                                           const bf16_t* __restrict__ res, bf16_t* __restrict__ xo, int ldx, TomeDims dm, int d,
                                                           int scale) {
  const int nch = d >> 3;
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)dm.B * dm.T * nch) return;
  const int c = (int)(item % nch);
  const long long btok = item / nch;
  const int b = (int)(btok / dm.T);
  const PlanLayout L = plan_layout(dm.B, dm.T, dm.r);
  const int row = min(max(plan[L.map + (size_t)btok], 0), dm.Tm - 1);
  const uint4 v = *(const uint4*)(y + ((size_t)b * dm.Tm + row) * ldy + c * 8);
  if (!res && !(scale && row < dm.nd)) {
    *(uint4*)(xo + (size_t)btok * ldx + c * 8) = v;            // a bitwise copy
    return;
  }
  float f[8];
  unpack8(v, f);
  if (scale && row < dm.nd) {
    const int* so = plan + L.seg_off + (size_t)b * (dm.nd + 1) + row;
    const float cntf = (float)(1 + min(max(so[1] - so[0], 0), dm.r));
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = f[e] / cntf;
  }
  if (res) {
    float g[8];
    unpack8(*(const uint4*)(res + (size_t)btok * ldx + c * 8), g);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = g[e] + f[e];
  }
  *(uint4*)(xo + (size_t)btok * ldx + c * 8) = pack8(f);
}

int check_dims(const char* what, int B, int T, int r, int d, TomeDims* dm) {
  E4T_REQUIRE(B >= 1 && T >= 4 && T % 4 == 0, "%s: B=%d T=%d (T must be a positive multiple of 4)", what, B, T);
  E4T_REQUIRE(T <= TOME_MAX_T, "%s: T=%d exceeds %d", what, T, TOME_MAX_T);
  const int nd = T / 4, ns = T - nd;
  E4T_REQUIRE(r >= 1 && r <= ns, "%s: r=%d outside [1, ns=%d]", what, r, ns);
  E4T_REQUIRE(d >= 8 && d % 8 == 0, "%s: d=%d must be a multiple of 8", what, d);
  *dm = TomeDims{B, T, nd, ns, r, T - r};
  return 0;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" size_t e4t_tome_plan_ints(int T, int r) {
  if (T < 4 || T % 4 || T > TOME_MAX_T || r < 1 || r > T - T / 4) return 0;
  return plan_layout(1, T, r).total;
}

extern "C" int e4t_tome_match(const void* x, int ldx, int B, int h, int w, int d, int r, const int* choice, int* plan, e4t_stream stream) {
  E4T_REQUIRE(x && plan, "tome_match: null operand");
  E4T_REQUIRE(h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0, "tome_match: grid %dx%d must have even sides", h, w);
  E4T_REQUIRE((long long)h * w <= TOME_MAX_T, "tome_match: T=%lld exceeds %d", (long long)h * w, TOME_MAX_T);
  E4T_REQUIRE(d >= 16 && d % 16 == 0, "tome_match: d=%d must be a multiple of 16", d);
  TomeDims dm;
  if (int rc = check_dims("tome_match", B, h * w, r, d, &dm)) return rc;
  E4T_REQUIRE(d <= 1280, "tome_match: d=%d exceeds 1280", d);
  E4T_REQUIRE(B <= 65535, "tome_match: B=%d exceeds 65535", B);
  E4T_REQUIRE(ldx >= d && ldx % 8 == 0 && aligned16(x), "tome_match: x rows must be 16-byte aligned (ldx=%d)", ldx);
  hipStream_t st = (hipStream_t)stream;
  const PlanLayout L = plan_layout(B, dm.T, r);
  int* src_tok = plan + L.src_tok;
  int* dst_tok = plan + L.dst_tok;
  float* norm = (float*)(plan + L.norm);
  float* node_max = (float*)(plan + L.node_max);
  int* node_idx = plan + L.node_idx;
  const bf16_t* xp = (const bf16_t*)x;
  const long long rows = (long long)B * dm.T;
  int P = 2;
  while (P < dm.ns) P <<= 1;
  const size_t sel_lds = (size_t)P * 8 + SEL_THREADS * 4;
  const size_t score_lds = (size_t)32 * (d + 8) * 2;
  static bool attr_set = false;
  if (!attr_set) {       // the largest request (T = 16384): 132 KiB of the CU's 160
    if (hipFuncSetAttribute((const void*)tome_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TOME_MAX_T * 8 + SEL_THREADS * 4) != hipSuccess)
      E4T_FAIL(-5, "tome_match: cannot reserve LDS for the selection kernel");
    if (hipFuncSetAttribute((const void*)tome_score_kernel<80>, hipFuncAttributeMaxDynamicSharedMemorySize, 32 * (1280 + 8) * 2) != hipSuccess)
      E4T_FAIL(-5, "tome_match: cannot reserve LDS for the score kernel");
    attr_set = true;
  }
  hipLaunchKernelGGL(tome_tokens_kernel, dim3(1), dim3(SEL_THREADS), 0, st, choice, h, w, src_tok, dst_tok);
  E4T_CHECK_LAUNCH("tome_tokens_kernel");
  hipLaunchKernelGGL(tome_norm_kernel, dim3((unsigned)cdivl(rows, 4)), dim3(256), 0, st, xp, ldx, rows, d, norm);
  E4T_CHECK_LAUNCH("tome_norm_kernel");
  const dim3 sg(cdiv(dm.ns, 128), B);
#define TOME_SCORE(NKS)                                                                                                                   \
  hipLaunchKernelGGL(tome_score_kernel<NKS>, sg, dim3(256), score_lds, st, xp, ldx, dm.T, dm.nd, dm.ns, d, (const float*)norm, (const int*)src_tok, \
                     (const int*)dst_tok, node_max, node_idx)
  const int nks = d / 16;
  if (nks <= 4) TOME_SCORE(4);
  else if (nks <= 20) TOME_SCORE(20);
  else if (nks <= 40) TOME_SCORE(40);
  else TOME_SCORE(80);
#undef TOME_SCORE
  E4T_CHECK_LAUNCH("tome_score_kernel");
  hipLaunchKernelGGL(tome_select_kernel, dim3(B), dim3(SEL_THREADS), sel_lds, st, dm, P, plan);
  E4T_CHECK_LAUNCH("tome_select_kernel");
  E4T_LOG_LAUNCH("tome_score_kernel<%d>|tome_match B%d %dx%d d%d r%d|%.0f|%.0f", nks <= 4 ? 4 : nks <= 20 ? 20 : nks <= 40 ? 40 : 80, B, h, w, d, r,
                 2.0 * rows * d + 8.0 * rows, 2.0 * B * (double)dm.ns * dm.nd * d);
  return 0;
}

extern "C" int e4t_tome_merge(const void* x, int ldx, const int* plan, void* y, int ldy, int B, int T, int r, int d, int mean, e4t_stream stream) {
  E4T_REQUIRE(x && plan && y, "tome_merge: null operand");
  TomeDims dm;
  if (int rc = check_dims("tome_merge", B, T, r, d, &dm)) return rc;
  E4T_REQUIRE(ldx >= d && ldy >= d && ldx % 8 == 0 && ldy % 8 == 0 && aligned16(x) && aligned16(y),
              "tome_merge: rows must be 16-byte aligned (ldx=%d ldy=%d)", ldx, ldy);
  const long long items = (long long)B * dm.Tm * (d / 8);
  hipLaunchKernelGGL(tome_merge_kernel, dim3((unsigned)cdivl(items, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, ldx, plan, (bf16_t*)y, ldy,
                     dm, d, mean);
  E4T_CHECK_LAUNCH("tome_merge_kernel");
  E4T_LOG_LAUNCH("tome_merge_kernel|B%d T%d r%d d%d mean%d|%.0f|0", B, T, r, d, mean, 2.0 * B * (double)(T + dm.Tm) * d);
  return 0;
}

extern "C" int e4t_tome_unmerge(const void* y, int ldy, const int* plan, const void* residual, void* x_out, int ldx, int B, int T, int r, int d,
                                int scale_inv_count, e4t_stream stream) {
  E4T_REQUIRE(y && plan && x_out, "tome_unmerge: null operand");
  TomeDims dm;
  if (int rc = check_dims("tome_unmerge", B, T, r, d, &dm)) return rc;
  E4T_REQUIRE(ldx >= d && ldy >= d && ldx % 8 == 0 && ldy % 8 == 0 && aligned16(y) && aligned16(x_out) && aligned16(residual),
              "tome_unmerge: rows must be 16-byte aligned (ldx=%d ldy=%d)", ldx, ldy);
  const long long items = (long long)B * T * (d / 8);
  hipLaunchKernelGGL(tome_unmerge_kernel, dim3((unsigned)cdivl(items, 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)y, ldy, plan,
                     (const bf16_t*)residual, (bf16_t*)x_out, ldx, dm, d, scale_inv_count);
  E4T_CHECK_LAUNCH("tome_unmerge_kernel");
  E4T_LOG_LAUNCH("tome_unmerge_kernel|B%d T%d r%d d%d res%d scale%d|%.0f|0", B, T, r, d, residual ? 1 : 0, scale_inv_count,
                 2.0 * B * (double)(T * (residual ? 2 : 1) + dm.Tm) * d);
  return 0;
}
