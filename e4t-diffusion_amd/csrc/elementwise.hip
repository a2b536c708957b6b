// Streaming (HBM-bound) helper kernels on NHWC bf16 activations: GEGLU, SiLU, transposes, weight
// relayout, 2x2 sum-pool (upsample backward), spatial mean (E4T UNet-feature pooling), sinusoidal
// timestep embedding, bicubic resize + CLIP normalisation + patchify, fused AdamW.
// All use 8/16-byte vector accesses with consecutive lanes on consecutive addresses.
#include "common.h"
#include "../../include/e4t_hip.h"

namespace {

// ---- GEGLU: h[m][j] = u[m][j] * gelu(u[m][H + j]),  u = proj(x) of width 2H  (attention.py:428-430) ----
__global__ __launch_bounds__(256) void geglu_fwd_kernel(const bf16_t* u, bf16_t* h, long long M, int H) {
  const int hc = H >> 3;
  const long long total = M * hc;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long m = i / hc; const int j = (int)(i - m * hc) * 8;
    float a[8], g[8];
    unpack8(*(const uint4*)(u + m * 2 * H + j), a);
    unpack8(*(const uint4*)(u + m * 2 * H + H + j), g);
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = geglu_f(a[k], g[k]);
    *(uint4*)(h + m * H + j) = pack8(a);
  }
}
// du[m][j] = dh * gelu(g) ; du[m][H+j] = dh * a * gelu'(g)
__global__ __launch_bounds__(256) void geglu_bwd_kernel(const bf16_t* u, const bf16_t* dh, bf16_t* du, long long M, int H) {
  const int hc = H >> 3;
  const long long total = M * hc;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long m = i / hc; const int j = (int)(i - m * hc) * 8;
    float a[8], g[8], d[8], oa[8], og[8];
    unpack8(*(const uint4*)(u + m * 2 * H + j), a);
    unpack8(*(const uint4*)(u + m * 2 * H + H + j), g);
    unpack8(*(const uint4*)(dh + m * H + j), d);
#pragma unroll
    for (int k = 0; k < 8; ++k) { oa[k] = geglu_da_f(d[k], g[k]); og[k] = geglu_dg_f(d[k], a[k], g[k]); }
    *(uint4*)(du + m * 2 * H + j) = pack8(oa);
    *(uint4*)(du + m * 2 * H + H + j) = pack8(og);
  }
}

// ---- unary: op 0 = silu, 1 = silu backward (dy, x) , 2 = gelu, 3 = gelu backward, 4 = leaky_relu(0.01), 5 = its backward,
//            6 = quick_gelu x*sigmoid(1.702 x) (CLIP text encoder of SD-1.x), 7 = its backward ----
__global__ __launch_bounds__(256) void unary_kernel(const bf16_t* x, const bf16_t* dy, bf16_t* y, long long n8, int op) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
    float f[8], d[8];
    unpack8(*(const uint4*)(x + i * 8), f);
    if (dy) unpack8(*(const uint4*)(dy + i * 8), d);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      switch (op) {
        case 0: f[k] = silu_f(f[k]); break;
        case 1: f[k] = d[k] * dsilu_f(f[k]); break;
        case 2: f[k] = gelu_f(f[k]); break;
        case 3: f[k] = d[k] * dgelu_f(f[k]); break;
        case 4: f[k] = f[k] > 0.f ? f[k] : 0.01f * f[k]; break;
        case 5: f[k] = f[k] > 0.f ? d[k] : 0.01f * d[k]; break;
        case 6: f[k] = f[k] / (1.f + __expf(-1.702f * f[k])); break;
        default: {
          // 1.702 x overflows for |x| > 2e38 where sg or 1 - sg is 0: inf * 0.  Clamped to a finite value the product is the 0 it stands for; below the clamp the bits are unchanged
          const float sg = 1.f / (1.f + __expf(-1.702f * f[k])), ax = fminf(fmaxf(1.702f * f[k], -3.0e38f), 3.0e38f);
          f[k] = d[k] * sg * (1.f + ax * (1.f - sg));
        } break;
      }
    }
    *(uint4*)(y + i * 8) = pack8(f);
  }
}

// ---- out = a + b (bf16), optional fp32 b ----
__global__ __launch_bounds__(256) void add_kernel(const bf16_t* a, const bf16_t* b, bf16_t* y, long long n8) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
    float f[8], g[8];
    unpack8(*(const uint4*)(a + i * 8), f);
    unpack8(*(const uint4*)(b + i * 8), g);
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] += g[k];
    *(uint4*)(y + i * 8) = pack8(f);
  }
}

// ---- batched 2-D transpose of bf16: in[b][R][C] (row stride ldi) -> out[b][C][R] (row stride ldo) ----
__global__ __launch_bounds__(256) void transpose_kernel(const bf16_t* in, bf16_t* out, int R, int C, int ldi, int ldo,
                                                        long long bsi, long long bso) {
  __shared__ bf16_t tile[64][66];
  const int b = blockIdx.z;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  in += (long long)b * bsi; out += (long long)b * bso;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rl = ty * 4 + k, r = r0 + rl, c = c0 + tx * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) tile[rl][tx * 4 + j] = (r < R && c + j < C) ? in[(long long)r * ldi + c + j] : (bf16_t)0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int cl = ty * 4 + k, c = c0 + cl, r = r0 + tx * 4;
    if (c < C)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (r + j < R) out[(long long)c * ldo + r + j] = tile[tx * 4 + j][cl];
  }
}

// ---- conv weight relayout: OIHW fp32 -> fwd [O][ky][kx][Ipad] bf16 and dgrad [I][2-ky][2-kx][Opad] bf16 ----
__global__ __launch_bounds__(256) void conv_weight_kernel(const float* w, bf16_t* wf, bf16_t* wd, int O, int I, int Ipad, int Opad) {
  const long long nf = (long long)O * 9 * Ipad, nd = (long long)I * 9 * Opad;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < nf + nd; idx += (long long)gridDim.x * 256) {
    if (idx < nf) {
      if (!wf) continue;
      const int i = (int)(idx % Ipad); const long long t = idx / Ipad;
      const int tap = (int)(t % 9), o = (int)(t / 9);
      wf[idx] = i < I ? f2bf(w[((long long)o * I + i) * 9 + tap]) : (bf16_t)0;
    } else {
      if (!wd) continue;
      const long long j = idx - nf;
      const int o = (int)(j % Opad); const long long t = j / Opad;
      const int tapd = (int)(t % 9), i = (int)(t / 9);
      const int tap = 8 - tapd;  // (2-ky)*3 + (2-kx)
      wd[j] = o < O ? f2bf(w[((long long)o * I + i) * 9 + tap]) : (bf16_t)0;
    }
  }
}

// ---- 2x2 sum pool: out[b][y][x][c] = sum in[b][2y+dy][2x+dx][c]  (backward of nearest x2 upsample) ----
__global__ __launch_bounds__(256) void sumpool2_kernel(const bf16_t* in, bf16_t* out, int Bn, int H, int W, int C) {
  const int c8 = C >> 3;
  const long long total = (long long)Bn * H * W * c8;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % c8) * 8; long long t = i / c8;
    const int x = (int)(t % W); t /= W; const int y = (int)(t % H); const int b = (int)(t / H);
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        float f[8];
        unpack8(*(const uint4*)(in + (((long long)b * 2 * H + 2 * y + dy) * 2 * W + 2 * x + dx) * C + c), f);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += f[k];
      }
    *(uint4*)(out + (((long long)b * H + y) * W + x) * C + c) = pack8(acc);
  }
}

// ---- spatial mean: out[b][coff + c] = mean_p x[b][p][c]  (encoder.py:147) ; grid (ceil(C/256), B) ----
// block = 1024 threads = 64 pixel groups x 16 lanes; each lane owns 4 channels of a 64-channel slab (8-byte loads,
// 128 B contiguous per pixel per 16 lanes); fixed-order LDS tree -> deterministic.
__global__ __launch_bounds__(1024) void spatial_mean_kernel(const bf16_t* x, float* out, int HW, int C, int ldo, int coff) {
  __shared__ float red[64][65];
  const int b = blockIdx.y, c0 = blockIdx.x * 64;
  const int lane = threadIdx.x & 15, pg = threadIdx.x >> 4;
  const int c = c0 + lane * 4;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    const bf16_t* p = x + (long long)b * HW * C + c;
    for (int i = pg; i < HW; i += 64) {
      float f[4];
      unpack4(*(const uint2*)(p + (long long)i * C), f);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += f[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[pg][lane * 4 + j] = s[j];
  __syncthreads();
  if (threadIdx.x < 64 && c0 + threadIdx.x < C) {
    float t = 0.f;
    for (int g = 0; g < 64; ++g) t += red[g][threadIdx.x];
    out[(long long)b * ldo + coff + c0 + threadIdx.x] = t / HW;
  }
}
// dx[b][p][c] = (base ? base : 0) + g[b][coff + c] / HW
__global__ __launch_bounds__(256) void spatial_mean_bwd_kernel(const float* g, const bf16_t* base, bf16_t* dx, int Bn, int HW, int C, int ldg, int coff) {
  const int c8 = C >> 3;
  const long long total = (long long)Bn * HW * c8;
  const float inv = 1.f / HW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % c8) * 8; const long long pix = i / c8; const int b = (int)(pix / HW);
    float f[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (base) unpack8(*(const uint4*)(base + pix * C + c), f);
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] += g[(long long)b * ldg + coff + c + k] * inv;
    *(uint4*)(dx + pix * C + c) = pack8(f);
  }
}

// ---- sinusoidal timestep embedding [cos | sin] (flip_sin_to_cos=True, freq_shift=0), bf16 out ----
__global__ void timestep_embed_kernel(const long long* t, bf16_t* out, int Bn, int dim) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int half = dim >> 1;
  if (i >= Bn * half) return;
  const int b = i / half, k = i - b * half;
  const float freq = __expf(-9.210340371976184f * (float)k / (float)half);
  const float ang = (float)t[b] * freq;
  out[(long long)b * dim + k] = f2bf(cosf(ang));
  out[(long long)b * dim + half + k] = f2bf(sinf(ang));
}

// ---- bicubic (A=-0.75, align_corners=True) 512->224 + (x+1)/2 + CLIP mean/std + patchify ----
// in: NCHW fp32 (B,3,Hin,Win) in [-1,1] ; out: bf16 [B*gh*gw][Kpad] with k = (c*P + py)*P + px  (conv1 weight order)
__device__ __forceinline__ void cubic_w(float t, float* w) {
  const float A = -0.75f;
  w[0] = ((A * (t + 1.f) - 5.f * A) * (t + 1.f) + 8.f * A) * (t + 1.f) - 4.f * A;
  w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  w[2] = ((A + 2.f) * (1.f - t) - (A + 3.f)) * (1.f - t) * (1.f - t) + 1.f;
  w[3] = 1.f - w[0] - w[1] - w[2];
}
__global__ __launch_bounds__(256) void clip_preprocess_kernel(const float* in, bf16_t* out, int Bn, int Hin, int Win, int S, int P, int Kpad) {
  const long long total = (long long)Bn * 3 * S * S;
  const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
  const float stdv[3] = {0.26862954f, 0.26130258f, 0.27577711f};
  const int g = S / P;
  const float sy = S > 1 ? (float)(Hin - 1) / (float)(S - 1) : 0.f, sx = S > 1 ? (float)(Win - 1) / (float)(S - 1) : 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int ox = (int)(i % S); long long t = i / S; const int oy = (int)(t % S); t /= S; const int c = (int)(t % 3); const int b = (int)(t / 3);
    const float fy = oy * sy, fx = ox * sx;
    const int iy = (int)floorf(fy), ix = (int)floorf(fx);
    float wy[4], wx[4];
    cubic_w(fy - iy, wy); cubic_w(fx - ix, wx);
    const float* src = in + ((long long)b * 3 + c) * Hin * Win;
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      int yy = iy - 1 + a; yy = yy < 0 ? 0 : (yy >= Hin ? Hin - 1 : yy);
      float r = 0.f;
#pragma unroll
      for (int bb = 0; bb < 4; ++bb) {
        int xx = ix - 1 + bb; xx = xx < 0 ? 0 : (xx >= Win ? Win - 1 : xx);
        r += wx[bb] * src[(long long)yy * Win + xx];
      }
      acc += wy[a] * r;
    }
    acc = ((acc + 1.f) * 0.5f - mean[c]) / stdv[c];
    const int py = oy / P, px = ox / P;
    const long long row = ((long long)b * g + py) * g + px;
    const int k = (c * P + (oy - py * P)) * P + (ox - px * P);
    out[row * Kpad + k] = f2bf(acc);
  }
}

// ---- fused AdamW over a flat fp32 buffer (torch.optim.AdamW semantics: decoupled weight decay) ----
// hyper != nullptr: lr, bc1, bc2_sqrt and the gradient scale are read from DEVICE memory ([4] floats) instead of the launch arguments,
// so that a captured (hipGraph) training step replays with the values of ITS step (e4t_adamw_hyper); same arithmetic either way.
// EMA of the weights in the same pass (adamw_ema_kernel): 36 B per parameter instead of 28 + 12 for a pass of its own.  One body, included
// into both kernels (adamw_kernel.inc).
__global__ __launch_bounds__(256) void adamw_kernel(float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2,
                                                    float eps, float wd, float bc1, float bc2_sqrt, float gscale, const float* hyper) {
  constexpr bool EMA = false;
  float* const ema = nullptr;
  float ema_w = 0.f;
#include "adamw_kernel.inc"
}
__global__ __launch_bounds__(256) void adamw_ema_kernel(float* p, const float* g, float* m, float* v, float* ema, long long n, float lr, float b1,
                                                        float b2, float eps, float wd, float bc1, float bc2_sqrt, float gscale, float ema_w,
                                                        const float* hyper) {
  constexpr bool EMA = true;
#include "adamw_kernel.inc"
}

// the EMA rule alone, for weights that something else updated (a stock optimiser over the native modules); w_dev != nullptr: w from device memory
__global__ __launch_bounds__(256) void ema_update_kernel(float* ema, const float* p, long long n, float w, const float* w_dev) {
  if (w_dev) w = w_dev[0];
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * 1024) {
    if (i + 4 <= n) {
      const float4 E = *(float4*)(ema + i), P = *(const float4*)(p + i);
      *(float4*)(ema + i) = make_float4(ema_f(E.x, P.x, w), ema_f(E.y, P.y, w), ema_f(E.z, P.z, w), ema_f(E.w, P.w, w));
    } else {
      for (long long j = i; j < n; ++j) ema[j] = ema_f(ema[j], p[j], w);
    }
  }
}

// ---- AdamW with block-wise 8-bit moments (the format is DEFINED by e4t/optimization.py: quantize_blockwise) ----
// m and v live as one byte each (an index into a sorted 256-entry codebook: signed for m, unsigned for v) plus one fp32 scale per 256
// elements: 16.06 B of HBM traffic per parameter instead of 28 (24.06 / 36 with the EMA) -- though as measured the kernel is bound by its per-element
// work (divisions, the two searches), not by HBM, and buys memory rather than time.  One wave64 owns one 256-element block, four
// consecutive elements per lane (a float4 of p and g, one packed word of each code buffer); the block maxima are wave reductions, so
// there is no barrier in the loop.  Per workgroup the two codebooks sit in LDS twice: sorted (dequantisation, the neighbour comparison)
// and as an implicit search tree in breadth-first order (node k's children are 2k and 2k + 1), whose level l occupies 2^l consecutive
// words: the eight reads of a search then fall on distinct banks or on one address, where a binary search over the sorted table would
// read words 128 / 64 / 32 apart (one bank) in its first levels.
// rank(y) = #{j < 255: code[j] < y}; q = rank or rank - 1, whichever is nearer in fp32, the lower index on a tie.
__device__ __forceinline__ int adam8_quant(const float* code, const float* tree, float x, float a) {
  const float y = a > 0.f ? x / a : 0.f;
  int k = 1;
#pragma unroll
  for (int l = 0; l < 8; ++l) k = 2 * k + (tree[k] < y ? 1 : 0);
  const int hi = k - 256, lo = hi > 0 ? hi - 1 : 0;
  return (y - code[lo] <= code[hi] - y) ? lo : hi;
}

template <bool EMA>
__global__ __launch_bounds__(256) void adamw8_kernel(float* p, const float* g, unsigned char* qm, unsigned char* qv, float* am, float* av, float* ema,
                                                     long long n, const float* code_m, const float* code_v, float lr, float b1, float b2, float eps,
                                                     float wd, float bc1, float bc2_sqrt, float gscale, float ema_w, const float* hyper) {
  __shared__ float s_cm[256], s_cv[256], s_tm[256], s_tv[256];
  {
    const int t = threadIdx.x;
    // tree node t (1..255) at level L = floor(log2 t), offset j = t - 2^L, is the sorted entry (2j + 1) * 2^(7 - L) - 1; node 0 is unused
    const int L = 31 - __clz(t | 1), idx = t ? (((2 * (t - (1 << L)) + 1) << (7 - L)) - 1) : 0;
    s_cm[t] = code_m[t]; s_cv[t] = code_v[t];
    s_tm[t] = code_m[idx]; s_tv[t] = code_v[idx];
  }
  __syncthreads();
  if (hyper) { lr = hyper[0]; bc1 = hyper[1]; bc2_sqrt = hyper[2]; gscale = hyper[3]; if constexpr (EMA) ema_w = hyper[4]; }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long nblk = (n + 255) / 256;
  for (long long blk = (long long)blockIdx.x * 4 + wave; blk < nblk; blk += (long long)gridDim.x * 4) {      // wave-uniform trip count
    const long long i = blk * 256 + lane * 4;
    const int cnt = i >= n ? 0 : (n - i >= 4 ? 4 : (int)(n - i));      // valid elements of this lane: 4, or fewer in the short last block
    const float a_m = am[blk], a_v = av[blk];
    float pp[4] = {0.f, 0.f, 0.f, 0.f}, gg[4] = {0.f, 0.f, 0.f, 0.f}, ee[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned wm = 0, wv = 0;
    if (cnt == 4) {
      const float4 P = *(const float4*)(p + i), G = *(const float4*)(g + i);
      pp[0] = P.x; pp[1] = P.y; pp[2] = P.z; pp[3] = P.w;
      gg[0] = G.x * gscale; gg[1] = G.y * gscale; gg[2] = G.z * gscale; gg[3] = G.w * gscale;
      wm = *(const unsigned*)(qm + i); wv = *(const unsigned*)(qv + i);
      if constexpr (EMA) { const float4 E = *(const float4*)(ema + i); ee[0] = E.x; ee[1] = E.y; ee[2] = E.z; ee[3] = E.w; }
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (k >= cnt) break;
        pp[k] = p[i + k]; gg[k] = g[i + k] * gscale;
        wm |= (unsigned)qm[i + k] << (8 * k); wv |= (unsigned)qv[i + k] << (8 * k);
        if constexpr (EMA) ee[k] = ema[i + k];
      }
    }
    float mm[4], vv[4], xm = 0.f, xv = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = k < cnt;      // a lane's missing elements carry zeros: they leave the block maxima alone
      mm[k] = ok ? s_cm[(wm >> (8 * k)) & 255] * a_m : 0.f;
      vv[k] = ok ? s_cv[(wv >> (8 * k)) & 255] * a_v : 0.f;
      // adamw_kernel.inc's arithmetic, in its order, with the contractions adamw_kernel compiles to (-ffp-contract=fast) written out: the decay
      // 1 - lr * wd, b * moment + (1 - b) * gradient term and decay * p - step are one fma each, and no other product feeds a sum, so nothing is
      // left for the compiler to fuse one way in one instantiation and another way in the other; p moves by the unquantised new moments
      mm[k] = fmaf(b1, mm[k], (1.f - b1) * gg[k]);
      vv[k] = fmaf(b2, vv[k], (1.f - b2) * gg[k] * gg[k]);
      const float denom = sqrtf(vv[k]) / bc2_sqrt + eps;
      // (adamw_kernel's last partial quad goes through its scalar loop, where decay * p - step stayed a product and a difference: the lane that
      // holds such a quad here is the same lane of the same buffer, and does the same, so that from zero moments EVERY p' is e4t_adamw's.
      // The empty asm keeps the backend from fusing that product: -ffp-contract=fast is a property of the whole file.)
      const float decay = fmaf(-lr, wd, 1.f), upd = (lr / bc1) * mm[k] / denom;
      float prod = decay * pp[k];
      asm volatile("" : "+v"(prod));
      pp[k] = cnt == 4 ? fmaf(decay, pp[k], -upd) : prod - upd;
      xm = fmaxf(xm, fabsf(mm[k])); xv = fmaxf(xv, vv[k]);
    }
    xm = wave_max(xm); xv = wave_max(xv);
    wm = 0; wv = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      wm |= (unsigned)adam8_quant(s_cm, s_tm, mm[k], xm) << (8 * k);
      wv |= (unsigned)adam8_quant(s_cv, s_tv, vv[k], xv) << (8 * k);
    }
    if (cnt == 4) {
      *(float4*)(p + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
      *(unsigned*)(qm + i) = wm; *(unsigned*)(qv + i) = wv;
      if constexpr (EMA)
        *(float4*)(ema + i) = make_float4(ema_f(ee[0], pp[0], ema_w), ema_f(ee[1], pp[1], ema_w), ema_f(ee[2], pp[2], ema_w), ema_f(ee[3], pp[3], ema_w));
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (k >= cnt) break;
        p[i + k] = pp[k];
        qm[i + k] = (unsigned char)(wm >> (8 * k)); qv[i + k] = (unsigned char)(wv >> (8 * k));
        if constexpr (EMA) ema[i + k] = ema_f(ee[k], pp[k], ema_w);
      }
    }
    if (lane == 0) { am[blk] = xm; av[blk] = xv; }
  }
}

// ---- AdamW of the E4T head's stacked first_linears weights with the gradient formed IN REGISTERS (round 6) ----
// The n = 129 weight gradients are rank-K products dW_i[r][c] = sum_k G[k][r] * Z[k][i*cols + c] (K = images of the step: the batch, or
// under data parallelism every rank's rows gathered; encoder.py:159-162): 845 MB of fp32 that the step used to write (batched GEMM), read
// back (AdamW) and clear (zero_grad).  Here a workgroup owns RB rows of one slot: a thread holds its 4 columns of the K x cols factor
// slice (bf16 -> fp32 registers, re-read from L2 by the cols / RB workgroups of the slot), the RB x K factor block of G sits in LDS
// and is read as broadcasts, and each element's gradient is a k-ordered fmaf chain in front of the same update arithmetic as
// adamw_kernel: 24 B of HBM traffic per parameter instead of 36, ~2 K FMAs per element on a kernel that stays HBM-bound.
template <int RB>
__global__ __launch_bounds__(320) void adamw_rank_kernel(float* p, float* m, float* v, const bf16_t* G, const bf16_t* Z, int rows, int cols, int K,
                                                         int ldg, long long ldz, float lr, float b1, float b2, float eps, float wd, float bc1,
                                                         float bc2_sqrt, float gscale, const float* hyper) {
  constexpr bool EMA = false;
  float* const ema = nullptr;
  float ema_w = 0.f;
#include "adamw_rank_kernel.inc"
}
template <int RB>
__global__ __launch_bounds__(320) void adamw_rank_ema_kernel(float* p, float* m, float* v, float* ema, const bf16_t* G, const bf16_t* Z, int rows, int cols,
                                                             int K, int ldg, long long ldz, float lr, float b1, float b2, float eps, float wd, float bc1,
                                                             float bc2_sqrt, float gscale, float ema_w, const float* hyper) {
  constexpr bool EMA = true;
#include "adamw_rank_kernel.inc"
}

// sum of squares of a flat fp32 buffer -> partial[blockIdx.x]
__global__ __launch_bounds__(256) void sumsq_kernel(const float* g, long long n, float* partial) {
  __shared__ float red[16];
  float s = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) s += g[i] * g[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

int grid_for(long long work, int cap = 2048) {
  long long b = (work + 255) / 256;
  if (b < 1) b = 1;
  return (int)(b > cap ? cap : b);
}

}  // namespace

extern "C" int e4t_geglu_fwd(const void* u, void* h, long long M, int H, e4t_stream s) {
  E4T_REQUIRE(u && h && M > 0 && H > 0 && H % 8 == 0, "geglu_fwd: bad arguments");
  E4T_LOG_LAUNCH("geglu_fwd_kernel|M%lld H%d|%.0f|0", M, H, 6.0 * (double)M * H);
  hipLaunchKernelGGL(geglu_fwd_kernel, dim3(grid_for(M * (H / 8))), dim3(256), 0, (hipStream_t)s, (const bf16_t*)u, (bf16_t*)h, M, H);
  E4T_CHECK_LAUNCH("geglu_fwd_kernel");
  return 0;
}
extern "C" int e4t_geglu_bwd(const void* u, const void* dh, void* du, long long M, int H, e4t_stream s) {
  E4T_REQUIRE(u && dh && du && M > 0 && H > 0 && H % 8 == 0, "geglu_bwd: bad arguments");
  E4T_LOG_LAUNCH("geglu_bwd_kernel|M%lld H%d|%.0f|0", M, H, 10.0 * (double)M * H);
  hipLaunchKernelGGL(geglu_bwd_kernel, dim3(grid_for(M * (H / 8))), dim3(256), 0, (hipStream_t)s, (const bf16_t*)u, (const bf16_t*)dh, (bf16_t*)du, M, H);
  E4T_CHECK_LAUNCH("geglu_bwd_kernel");
  return 0;
}
extern "C" int e4t_unary(const void* x, const void* dy, void* y, long long n, int op, e4t_stream s) {
  E4T_REQUIRE(x && y && n > 0 && n % 8 == 0 && op >= 0 && op <= 7, "unary: bad arguments (n %% 8 == 0 required)");
  E4T_REQUIRE(((op & 1) == 0) || dy, "unary: backward ops need dy");
  hipLaunchKernelGGL(unary_kernel, dim3(grid_for(n / 8)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)x, (const bf16_t*)((op & 1) ? dy : nullptr), (bf16_t*)y, n / 8, op);
  E4T_CHECK_LAUNCH("unary_kernel");
  return 0;
}
extern "C" int e4t_add(const void* a, const void* b, void* y, long long n, e4t_stream s) {
  E4T_REQUIRE(a && b && y && n > 0 && n % 8 == 0, "add: bad arguments");
  hipLaunchKernelGGL(add_kernel, dim3(grid_for(n / 8)), dim3(256), 0, (hipStream_t)s, (const bf16_t*)a, (const bf16_t*)b, (bf16_t*)y, n / 8);
  E4T_CHECK_LAUNCH("add_kernel");
  return 0;
}
// Classifier-free guidance + one linear scheduler update in a single pass (pipeline_stable_diffusion_e4t.py:209-214):
//   eps = cfg ? u + g*(c - u) : pred ;  out = c_sample*sample + c_pred*eps (+ c_noise*noise)
// coef = {g, c_sample, c_pred, c_noise} lives in device memory so a captured hipGraph of the step can be replayed with
// new coefficients.  pred may be given in the UNet's NHWC output layout ([B][HW][C]); sample / noise / out are NCHW.
__global__ __launch_bounds__(256) void guided_step_kernel(const float* __restrict__ pred, const float* __restrict__ sample, const float* __restrict__ noise,
                                                          float* __restrict__ out, const float* __restrict__ coef, int B, int C, int HW, int cfg, int nhwc) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n = (long long)B * C * HW;
  if (i >= n) return;
  const float g = coef[0], cs = coef[1], cp = coef[2], cn = coef[3];
  long long j = i;
  if (nhwc) {
    const int p = (int)(i % HW), c = (int)((i / HW) % C), b = (int)(i / ((long long)HW * C));
    j = ((long long)b * HW + p) * C + c;
  }
  float e = pred[j];
  if (cfg) {
    const float t = pred[j + n];
    e = e + g * (t - e);
  }
  float o = cs * sample[i] + cp * e;
  if (noise) o += cn * noise[i];
  out[i] = o;
}
extern "C" int e4t_guided_step(const float* pred, const float* sample, const float* noise, float* out, const float* coef,
                               int B, int C, int HW, int cfg, int pred_nhwc, e4t_stream s) {
  E4T_REQUIRE(pred && sample && out && coef && B > 0 && C > 0 && HW > 0, "guided_step: bad arguments");
  const long long n = (long long)B * C * HW;
  hipLaunchKernelGGL(guided_step_kernel, dim3((unsigned)cdivl(n, 256)), dim3(256), 0, (hipStream_t)s, pred, sample, noise, out, coef, B, C, HW, cfg, pred_nhwc);
  E4T_CHECK_LAUNCH("guided_step_kernel");
  return 0;
}
// Per-image statistics of the guided value for guidance rescale (e4t_guidance_stats in the header): one workgroup of 1024
// threads per image, two passes over the image's N = C*HW values (means, then squared deviations from them; the second pass
// reads what the first left in L2).  A one-pass sum / sum of squares loses the deviation of an image whose mean is large
// against it.  An image's slab is the same N contiguous values in NCHW and NHWC, and a sum does not care which element is
// which, so both layouts walk the slab in storage order.  Every thread adds its strided elements in index order and block_sum
// combines in a fixed order: no atomics, the same bits on every call.  V = 4: 16-byte loads (N % 4 == 0, aligned pred).
__device__ __forceinline__ float guide_e0(float u, float t, float c, float g, float g_id, int branches) {
  if (branches == 3) return __fmaf_rn(g_id, c - t, __fmaf_rn(g, t - u, u));
  return u + g * (t - u);                                  // branches == 2: t is c; sampler_step_kernel's expression
}
template <int V>
__global__ __launch_bounds__(1024) void guidance_stats_kernel(const float* __restrict__ pred, const float* __restrict__ gp, float* __restrict__ gstat,
                                                              long long n, int N, int branches) {
  __shared__ float red[32];
  const float g = gp[0], g_id = gp[1], phi = gp[2];
  const float* u = pred + (long long)blockIdx.x * N;       // branch 0 of this image; branch r is at u + r*n
  const float* c = u + (branches - 1) * n;
  float vu[V], vt[V], vc[V];
  float se = 0.f, sc = 0.f;
  for (int i = threadIdx.x * V; i < N; i += 1024 * V) {
    if constexpr (V == 4) {
      *(float4*)vu = *(const float4*)(u + i);
      *(float4*)vt = *(const float4*)(u + n + i);
      *(float4*)vc = *(const float4*)(c + i);
    } else {
      vu[0] = u[i], vt[0] = u[n + i], vc[0] = c[i];
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      se += guide_e0(vu[v], vt[v], vc[v], g, g_id, branches);
      sc += vc[v];
    }
  }
  const float me = block_sum(se, red) / (float)N, mc = block_sum(sc, red + 16) / (float)N;
  float qe = 0.f, qc = 0.f;
  for (int i = threadIdx.x * V; i < N; i += 1024 * V) {
    if constexpr (V == 4) {
      *(float4*)vu = *(const float4*)(u + i);
      *(float4*)vt = *(const float4*)(u + n + i);
      *(float4*)vc = *(const float4*)(c + i);
    } else {
      vu[0] = u[i], vt[0] = u[n + i], vc[0] = c[i];
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const float de = guide_e0(vu[v], vt[v], vc[v], g, g_id, branches) - me, dc = vc[v] - mc;
      qe = __fmaf_rn(de, de, qe);
      qc = __fmaf_rn(dc, dc, qc);
    }
  }
  qe = block_sum(qe, red);
  qc = block_sum(qc, red + 16);
  if (threadIdx.x == 0) {
    const float s_e = sqrtf(qe / (float)(N - 1)), s_c = sqrtf(qc / (float)(N - 1));
    const float ratio = s_c / s_e;
    const float f = (s_e == 0.f || !isfinite(ratio)) ? 1.f : (1.f - phi) + phi * ratio;
    float* o = gstat + (long long)blockIdx.x * E4T_GUIDE_STATS;
    o[0] = f, o[1] = s_c, o[2] = s_e, o[3] = me;
  }
}
extern "C" int e4t_guidance_stats(const float* pred, const float* gp, float* gstat, int B, int C, int HW, int branches, int pred_nhwc, e4t_stream s) {
  E4T_REQUIRE(pred, "guidance_stats: pred is null");
  E4T_REQUIRE(gp, "guidance_stats: gp is null");
  E4T_REQUIRE(gstat, "guidance_stats: gstat is null");
  E4T_REQUIRE(branches == 2 || branches == 3, "guidance_stats: branches = %d (2: [u | c], 3: [u | k | c])", branches);
  E4T_REQUIRE(B > 0 && C > 0 && HW > 0 && (long long)C * HW <= 0x7fffffffLL, "guidance_stats: B = %d, C = %d, HW = %d", B, C, HW);
  E4T_REQUIRE((long long)C * HW >= 2, "guidance_stats: N = C*HW = %lld values per image (an unbiased deviation needs N >= 2)", (long long)C * HW);
  (void)pred_nhwc;                                         // storage order: see the kernel
  const int N = C * HW;
  const long long n = (long long)B * N;
  if (N % 4 == 0 && ((uintptr_t)pred & 15) == 0)
    hipLaunchKernelGGL(guidance_stats_kernel<4>, dim3(B), dim3(1024), 0, (hipStream_t)s, pred, gp, gstat, n, N, branches);
  else
    hipLaunchKernelGGL(guidance_stats_kernel<1>, dim3(B), dim3(1024), 0, (hipStream_t)s, pred, gp, gstat, n, N, branches);
  E4T_CHECK_LAUNCH("guidance_stats_kernel");
  return 0;
}
// Guidance + one step of any linear sampler (DDIM, PLMS, LMS, Euler, Euler-ancestral, DPM-Solver++ 2M) in a single pass.
// The row contract is the header's (e4t_sampler_step).  Every thread owns one element index across x, out, hist, saved
// and x_in, so reading the old values before writing the new ones needs no synchronisation and x may alias out.
// Terms whose coefficient is 0 are skipped (uniform branch on a row value), which keeps a DDIM row's arithmetic exactly
// guided_step_kernel's: same expressions in the same order, so the same contraction.
// BLEND (e4t_sampler_step_edit): the finished o is mixed with the original latent re-noised to the level of the row's output,
// y = a_keep*x0 + s_keep*n0 with (a_keep, s_keep) = row[14], row[15], weighted by keep; both entry points are instances of
// this one body, and everything up to the mix is the same code, so the plain entry point's arithmetic cannot drift.
// GUIDED (e4t_sampler_step_guided): g comes from gp instead of row[0], a third branch [u | k | c] adds the identity term
// g_id*(c - k), and the guided value is scaled by the image's rescale factor gstat[b][0] (e4t_guidance_stats) when gstat is
// given.  With branches == 2 and no gstat the guidance line is the one the plain entry points run, so the bits are theirs.
template <bool BLEND, bool GUIDED>
__global__ __launch_bounds__(256) void sampler_step_kernel(const float* __restrict__ pred, const float* x, float* out, float* hist, float* saved,
                                                           const float* __restrict__ noise, float* x_in, const float* __restrict__ row,
                                                           const float* __restrict__ keep, const float* __restrict__ x0, const float* __restrict__ n0,
                                                           const float* __restrict__ gp, const float* __restrict__ gstat,
                                                           int B, int C, int HW, int K, int cfg, int nhwc, int x_in_copies,
                                                           int keep_per_image, int x0_per_image, int branches) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n = (long long)B * C * HW;
  if (i >= n) return;
  const float g = GUIDED ? gp[0] : row[0], a_e = row[1], a_x = row[2], c_x = row[3], c_s = row[4], c_m = row[5], c_n = row[6], k_in = row[7];
  const int w = (int)row[8], save_x = row[9] != 0.f;
  long long j = i;
  if (nhwc) {
    const int p = (int)(i % HW), c = (int)((i / HW) % C), b = (int)(i / ((long long)HW * C));
    j = ((long long)b * HW + p) * C + c;
  }
  float e = pred[j];
  if (cfg) {
    const float t = pred[j + n];
    if (GUIDED && branches == 3) e = __fmaf_rn(gp[1], pred[j + 2 * n] - t, __fmaf_rn(g, t - e, e));
    else e = e + g * (t - e);
  }
  if constexpr (GUIDED) {
    if (gstat) e *= gstat[(i / ((long long)C * HW)) * E4T_GUIDE_STATS];
  }
  const float xv = x[i];
  float m = a_e * e;
  if (a_x != 0.f) m = __fmaf_rn(a_x, xv, m);
  float o = c_x * xv + c_m * m;
  if (c_s != 0.f && saved) o = __fmaf_rn(c_s, saved[i], o);
  for (int k = 0; k < K; ++k) {
    const float ck = row[10 + k];
    if (ck != 0.f) o = __fmaf_rn(ck, hist[k * n + i], o);
  }
  if (noise && c_n != 0.f) o += c_n * noise[i];
  if (w >= 0 && w < K) hist[w * n + i] = m;
  if (save_x && saved) saved[i] = xv;
  if constexpr (BLEND) {
    const long long chw = (long long)C * HW;
    const float kp = keep[(keep_per_image ? (i / chw) * HW : 0) + i % HW];
    const float y = __fmaf_rn(row[15], n0[i], row[14] * x0[x0_per_image ? i : i % chw]);
    o = __fmaf_rn(kp, y, (1.f - kp) * o);
  }
  out[i] = o;
  if (x_in_copies > 0) {
    const float v = k_in * o;
    x_in[i] = v;
    if (x_in_copies > 1) x_in[n + i] = v;
    if (x_in_copies > 2) x_in[2 * n + i] = v;
  }
}
extern "C" int e4t_sampler_step(const float* pred, const float* x, float* out, float* hist, float* saved, const float* noise, float* x_in,
                                const float* row, int B, int C, int HW, int K, int cfg, int pred_nhwc, int x_in_copies, e4t_stream s) {
  E4T_REQUIRE(pred && x && out && row && B > 0 && C > 0 && HW > 0, "sampler_step: bad arguments");
  E4T_REQUIRE(K >= 0 && K <= E4T_SAMPLER_MAX_HIST && (K == 0 || hist), "sampler_step: K = %d history slots (0..%d, hist required when K > 0)", K, E4T_SAMPLER_MAX_HIST);
  E4T_REQUIRE(x_in_copies >= 0 && x_in_copies <= 2 && (x_in_copies == 0 || x_in), "sampler_step: x_in_copies = %d (0..2, x_in required when > 0)", x_in_copies);
  const long long n = (long long)B * C * HW;
  hipLaunchKernelGGL((sampler_step_kernel<false, false>), dim3((unsigned)cdivl(n, 256)), dim3(256), 0, (hipStream_t)s, pred, x, out, hist, saved, noise, x_in, row,
                     nullptr, nullptr, nullptr, nullptr, nullptr, B, C, HW, K, cfg, pred_nhwc, x_in_copies, 0, 0, 2);
  E4T_CHECK_LAUNCH("sampler_step_kernel");
  return 0;
}
extern "C" int e4t_sampler_step_edit(const float* pred, const float* x, float* out, float* hist, float* saved, const float* noise, float* x_in,
                                     const float* row, const float* keep, const float* x0, const float* n0, int B, int C, int HW, int K, int cfg,
                                     int pred_nhwc, int x_in_copies, int keep_per_image, int x0_per_image, e4t_stream s) {
  E4T_REQUIRE(pred && x && out && row && B > 0 && C > 0 && HW > 0, "sampler_step_edit: bad arguments");
  E4T_REQUIRE(keep && x0 && n0, "sampler_step_edit: keep, x0 and n0 are required");
  E4T_REQUIRE((keep_per_image == 0 || keep_per_image == 1) && (x0_per_image == 0 || x0_per_image == 1),
              "sampler_step_edit: keep_per_image = %d, x0_per_image = %d (0 or 1)", keep_per_image, x0_per_image);
  E4T_REQUIRE(K >= 0 && K <= E4T_SAMPLER_MAX_HIST && (K == 0 || hist), "sampler_step_edit: K = %d history slots (0..%d, hist required when K > 0)", K, E4T_SAMPLER_MAX_HIST);
  E4T_REQUIRE(x_in_copies >= 0 && x_in_copies <= 2 && (x_in_copies == 0 || x_in), "sampler_step_edit: x_in_copies = %d (0..2, x_in required when > 0)", x_in_copies);
  const long long n = (long long)B * C * HW;
  hipLaunchKernelGGL((sampler_step_kernel<true, false>), dim3((unsigned)cdivl(n, 256)), dim3(256), 0, (hipStream_t)s, pred, x, out, hist, saved, noise, x_in, row,
                     keep, x0, n0, nullptr, nullptr, B, C, HW, K, cfg, pred_nhwc, x_in_copies, keep_per_image, x0_per_image, 2);
  E4T_CHECK_LAUNCH("sampler_step_edit_kernel");
  return 0;
}
extern "C" int e4t_sampler_step_guided(const float* pred, const float* x, float* out, float* hist, float* saved, const float* noise, float* x_in,
                                       const float* row, const float* gp, const float* gstat, const float* keep, const float* x0, const float* n0,
                                       int B, int C, int HW, int K, int branches, int pred_nhwc, int x_in_copies, int keep_per_image,
                                       int x0_per_image, e4t_stream s) {
  E4T_REQUIRE(pred && x && out && row && gp && B > 0 && C > 0 && HW > 0, "sampler_step_guided: bad arguments");
  E4T_REQUIRE(branches == 2 || branches == 3, "sampler_step_guided: branches = %d (2: [u | c], 3: [u | k | c])", branches);
  const bool blend = keep && x0 && n0;
  E4T_REQUIRE(blend || (!keep && !x0 && !n0), "sampler_step_guided: keep, x0 and n0 are given together or not at all");
  E4T_REQUIRE((keep_per_image == 0 || keep_per_image == 1) && (x0_per_image == 0 || x0_per_image == 1),
              "sampler_step_guided: keep_per_image = %d, x0_per_image = %d (0 or 1)", keep_per_image, x0_per_image);
  E4T_REQUIRE(K >= 0 && K <= E4T_SAMPLER_MAX_HIST && (K == 0 || hist), "sampler_step_guided: K = %d history slots (0..%d, hist required when K > 0)", K, E4T_SAMPLER_MAX_HIST);
  E4T_REQUIRE(x_in_copies >= 0 && x_in_copies <= 3 && (x_in_copies == 0 || x_in), "sampler_step_guided: x_in_copies = %d (0..3, x_in required when > 0)", x_in_copies);
  const long long n = (long long)B * C * HW;
  if (blend)
    hipLaunchKernelGGL((sampler_step_kernel<true, true>), dim3((unsigned)cdivl(n, 256)), dim3(256), 0, (hipStream_t)s, pred, x, out, hist, saved, noise, x_in,
                       row, keep, x0, n0, gp, gstat, B, C, HW, K, 1, pred_nhwc, x_in_copies, keep_per_image, x0_per_image, branches);
  else
    hipLaunchKernelGGL((sampler_step_kernel<false, true>), dim3((unsigned)cdivl(n, 256)), dim3(256), 0, (hipStream_t)s, pred, x, out, hist, saved, noise, x_in,
                       row, nullptr, nullptr, nullptr, gp, gstat, B, C, HW, K, 1, pred_nhwc, x_in_copies, 0, 0, branches);
  E4T_CHECK_LAUNCH("sampler_step_guided_kernel");
  return 0;
}
extern "C" int e4t_transpose(const void* in, void* out, int batch, int R, int C, int ldi, int ldo, long long bsi, long long bso, e4t_stream s) {
  E4T_REQUIRE(in && out && batch > 0 && R > 0 && C > 0 && ldi >= C && ldo >= R, "transpose: bad arguments");
  E4T_REQUIRE(batch <= 65535 && cdiv(R, 64) <= 65535, "transpose: batch = %d, R = %d (at most 65535 batches and 65535 row tiles of 64: grid.z, grid.y)", batch, R);
  hipLaunchKernelGGL(transpose_kernel, dim3(cdiv(C, 64), cdiv(R, 64), batch), dim3(256), 0, (hipStream_t)s, (const bf16_t*)in, (bf16_t*)out, R, C, ldi, ldo, bsi, bso);
  E4T_CHECK_LAUNCH("transpose_kernel");
  return 0;
}
extern "C" int e4t_conv_weight_prepare(const float* w_oihw, void* w_fwd, void* w_dgrad, int O, int I, int Ipad, int Opad, e4t_stream s) {
  E4T_REQUIRE(w_oihw && (w_fwd || w_dgrad) && O > 0 && I > 0 && Ipad >= I && Opad >= O, "conv_weight_prepare: bad arguments");
  const long long n = (long long)O * 9 * Ipad + (long long)I * 9 * Opad;
  hipLaunchKernelGGL(conv_weight_kernel, dim3(grid_for(n, 4096)), dim3(256), 0, (hipStream_t)s, w_oihw, (bf16_t*)w_fwd, (bf16_t*)w_dgrad, O, I, Ipad, Opad);
  E4T_CHECK_LAUNCH("conv_weight_kernel");
  return 0;
}
extern "C" int e4t_sumpool2(const void* in, void* out, int Bn, int H, int W, int C, e4t_stream s) {
  E4T_REQUIRE(in && out && Bn > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "sumpool2: bad arguments (C > 0, C %% 8 == 0)");
  hipLaunchKernelGGL(sumpool2_kernel, dim3(grid_for((long long)Bn * H * W * (C / 8))), dim3(256), 0, (hipStream_t)s, (const bf16_t*)in, (bf16_t*)out, Bn, H, W, C);
  E4T_CHECK_LAUNCH("sumpool2_kernel");
  return 0;
}
extern "C" int e4t_spatial_mean(const void* x, float* out, int Bn, int HW, int C, int ldo, int coff, e4t_stream s) {
  E4T_REQUIRE(x && out && Bn > 0 && HW > 0 && C > 0 && C % 4 == 0, "spatial_mean: bad arguments (C %% 4 == 0)");
  E4T_REQUIRE(coff >= 0 && (long long)ldo >= (long long)coff + C, "spatial_mean: coff = %d, ldo = %d (coff >= 0 and ldo >= coff + C = %lld: the slice lies inside a row of out)",
              coff, ldo, (long long)coff + C);
  E4T_REQUIRE(Bn <= 65535, "spatial_mean: B = %d (at most 65535 images: grid.y)", Bn);
  hipLaunchKernelGGL(spatial_mean_kernel, dim3(cdiv(C, 64), Bn), dim3(1024), 0, (hipStream_t)s, (const bf16_t*)x, out, HW, C, ldo, coff);
  E4T_CHECK_LAUNCH("spatial_mean_kernel");
  return 0;
}
extern "C" int e4t_spatial_mean_bwd(const float* g, const void* base, void* dx, int Bn, int HW, int C, int ldg, int coff, e4t_stream s) {
  E4T_REQUIRE(g && dx && Bn > 0 && HW > 0 && C > 0 && C % 8 == 0, "spatial_mean_bwd: bad arguments (C > 0, C %% 8 == 0)");
  E4T_REQUIRE(coff >= 0 && (long long)ldg >= (long long)coff + C, "spatial_mean_bwd: coff = %d, ldg = %d (coff >= 0 and ldg >= coff + C = %lld: the slice lies inside a row of g)",
              coff, ldg, (long long)coff + C);
  E4T_REQUIRE(Bn <= 65535, "spatial_mean_bwd: B = %d (at most 65535 images, as e4t_spatial_mean)", Bn);
  hipLaunchKernelGGL(spatial_mean_bwd_kernel, dim3(grid_for((long long)Bn * HW * (C / 8))), dim3(256), 0, (hipStream_t)s, g, (const bf16_t*)base, (bf16_t*)dx, Bn, HW, C, ldg, coff);
  E4T_CHECK_LAUNCH("spatial_mean_bwd_kernel");
  return 0;
}
extern "C" int e4t_timestep_embedding(const long long* t, void* out, int Bn, int dim, e4t_stream s) {
  E4T_REQUIRE(t && out && Bn > 0 && dim > 0 && dim % 2 == 0, "timestep_embedding: bad arguments");
  hipLaunchKernelGGL(timestep_embed_kernel, dim3(cdiv(Bn * dim / 2, 256)), dim3(256), 0, (hipStream_t)s, t, (bf16_t*)out, Bn, dim);
  E4T_CHECK_LAUNCH("timestep_embed_kernel");
  return 0;
}
extern "C" int e4t_clip_preprocess(const float* pixels_nchw, void* patches, int Bn, int Hin, int Win, int S, int P, int Kpad, e4t_stream s) {
  E4T_REQUIRE(pixels_nchw && patches && Bn > 0, "clip_preprocess: bad arguments");
  E4T_REQUIRE(P > 0 && S > 0 && Hin > 0 && Win > 0, "clip_preprocess: P = %d, S = %d, Hin = %d, Win = %d must be positive", P, S, Hin, Win);      // before the modulo: P = 0 would trap on the host
  E4T_REQUIRE(S % P == 0 && (long long)Kpad >= 3LL * P * P, "clip_preprocess: bad arguments (S %% P == 0, Kpad >= 3 * P * P)");
  hipLaunchKernelGGL(clip_preprocess_kernel, dim3(grid_for((long long)Bn * 3 * S * S)), dim3(256), 0, (hipStream_t)s, pixels_nchw, (bf16_t*)patches, Bn, Hin, Win, S, P, Kpad);
  E4T_CHECK_LAUNCH("clip_preprocess_kernel");
  return 0;
}
extern "C" int e4t_adamw(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                         float weight_decay, int step, float grad_scale, e4t_stream s) {
  E4T_REQUIRE(p && g && m && v && n > 0 && step >= 1, "adamw: bad arguments");
  E4T_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "adamw: buffers must be 16-B aligned");
  const float bc1 = 1.f - powf(beta1, (float)step), bc2 = sqrtf(1.f - powf(beta2, (float)step));
  E4T_LOG_LAUNCH("adamw_kernel|n%lld|%.0f|0", (long long)n, 28.0 * (double)n);
  hipLaunchKernelGGL(adamw_kernel, dim3(grid_for((n + 3) / 4, 4096)), dim3(256), 0, (hipStream_t)s, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2, grad_scale,
                     (const float*)nullptr);
  E4T_CHECK_LAUNCH("adamw_kernel");
  return 0;
}
extern "C" int e4t_adamw_hyper(float* p, const float* g, float* m, float* v, long long n, const float* hyper_dev, float beta1, float beta2, float eps,
                               float weight_decay, e4t_stream s) {
  E4T_REQUIRE(p && g && m && v && hyper_dev && n > 0, "adamw_hyper: bad arguments");
  E4T_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)hyper_dev) & 15) == 0, "adamw_hyper: buffers must be 16-B aligned");
  E4T_LOG_LAUNCH("adamw_kernel|n%lld|%.0f|0", (long long)n, 28.0 * (double)n);
  hipLaunchKernelGGL(adamw_kernel, dim3(grid_for((n + 3) / 4, 4096)), dim3(256), 0, (hipStream_t)s, p, g, m, v, n, 0.f, beta1, beta2, eps, weight_decay, 1.f, 1.f, 1.f, hyper_dev);
  E4T_CHECK_LAUNCH("adamw_kernel");
  return 0;
}
extern "C" int e4t_adamw_rank(float* p, float* m, float* v, const void* G, const void* Z, int n, int rows, int cols, int K, int ldg, long long ldz,
                              float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, const float* hyper_dev,
                              e4t_stream s) {
  E4T_REQUIRE(p && m && v && G && Z && n > 0 && rows > 0 && cols > 0 && K > 0 && (hyper_dev || step >= 1), "adamw_rank: bad arguments");
  E4T_REQUIRE(cols % 4 == 0 && ldz % 4 == 0 && ldg >= rows && ldz >= (long long)n * cols, "adamw_rank: cols and the Z row stride must be multiples of 4");
  E4T_REQUIRE((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) == 0 && ((uintptr_t)Z & 7) == 0 && ((uintptr_t)hyper_dev & 15) == 0,
              "adamw_rank: buffers must be 16-B (factors 8-B) aligned");
  const float bc1 = hyper_dev ? 1.f : 1.f - powf(beta1, (float)step), bc2 = hyper_dev ? 1.f : sqrtf(1.f - powf(beta2, (float)step));
  constexpr int RB = 8;
  const int threads = min(320, (cols / 4 + 63) / 64 * 64);
  // algorithmic bytes: p, m, v read and written; the factors are L2 traffic
  E4T_LOG_LAUNCH("adamw_rank_kernel<%d>|n%d rows%d cols%d K%d|%.0f|%.0f", RB, n, rows, cols, K, 24.0 * n * rows * cols, 2.0 * n * rows * (double)cols * K);
  hipLaunchKernelGGL((adamw_rank_kernel<RB>), dim3(cdiv(rows, RB), n), dim3(threads), 0, (hipStream_t)s, p, m, v, (const bf16_t*)G, (const bf16_t*)Z, rows, cols, K,
                     ldg, ldz, hyper_dev ? 0.f : lr, beta1, beta2, eps, weight_decay, bc1, bc2, hyper_dev ? 1.f : grad_scale, hyper_dev);
  E4T_CHECK_LAUNCH("adamw_rank_kernel");
  return 0;
}
extern "C" int e4t_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, long long n, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int step, float grad_scale, float ema_w, const float* hyper_dev, e4t_stream s) {
  E4T_REQUIRE(p && g && m && v && ema && n > 0 && (hyper_dev || step >= 1), "adamw_ema: bad arguments");
  E4T_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema | (uintptr_t)hyper_dev) & 15) == 0,
              "adamw_ema: buffers must be 16-B aligned");
  const float bc1 = hyper_dev ? 1.f : 1.f - powf(beta1, (float)step), bc2 = hyper_dev ? 1.f : sqrtf(1.f - powf(beta2, (float)step));
  E4T_LOG_LAUNCH("adamw_ema_kernel|n%lld|%.0f|0", (long long)n, 36.0 * (double)n);
  hipLaunchKernelGGL(adamw_ema_kernel, dim3(grid_for((n + 3) / 4, 4096)), dim3(256), 0, (hipStream_t)s, p, g, m, v, ema, n, hyper_dev ? 0.f : lr, beta1, beta2, eps,
                     weight_decay, bc1, bc2, hyper_dev ? 1.f : grad_scale, hyper_dev ? 0.f : ema_w, hyper_dev);
  E4T_CHECK_LAUNCH("adamw_ema_kernel");
  return 0;
}
extern "C" int e4t_adamw8(float* p, const float* g, void* qm, void* qv, float* absmax_m, float* absmax_v, float* ema, long long n, const float* code_m,
                          const float* code_v, float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, float ema_w,
                          const float* hyper_dev, e4t_stream s) {
  E4T_REQUIRE(p && g && qm && qv && absmax_m && absmax_v && code_m && code_v && n > 0 && (hyper_dev || step >= 1), "adamw8: bad arguments");
  E4T_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)ema | (uintptr_t)hyper_dev) & 15) == 0, "adamw8: p, g, ema and hyper_dev must be 16-B aligned");
  E4T_REQUIRE((((uintptr_t)qm | (uintptr_t)qv | (uintptr_t)absmax_m | (uintptr_t)absmax_v | (uintptr_t)code_m | (uintptr_t)code_v) & 3) == 0,
              "adamw8: codes, scales and codebooks must be 4-B aligned");
  const float bc1 = hyper_dev ? 1.f : 1.f - powf(beta1, (float)step), bc2 = hyper_dev ? 1.f : sqrtf(1.f - powf(beta2, (float)step));
  const int grid = grid_for((n + 3) / 4, 4096);      // 1024 elements (four blocks of 256, one per wave) per workgroup and trip, as adamw_kernel
  const double bytes = 16.0 * (double)n + 16.0 * (double)((n + 255) / 256) + (ema ? 8.0 * (double)n : 0.0);
#define E4T_ADAMW8_ARGS                                                                                                                                      \
  p, g, (unsigned char*)qm, (unsigned char*)qv, absmax_m, absmax_v, ema, n, code_m, code_v, hyper_dev ? 0.f : lr, beta1, beta2, eps, weight_decay, bc1, bc2, \
      hyper_dev ? 1.f : grad_scale, hyper_dev ? 0.f : ema_w, hyper_dev
  if (ema) {
    E4T_LOG_LAUNCH("adamw8_ema_kernel|n%lld grid%d|%.0f|0", (long long)n, grid, bytes);
    hipLaunchKernelGGL(adamw8_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)s, E4T_ADAMW8_ARGS);
    E4T_CHECK_LAUNCH("adamw8_ema_kernel");
  } else {
    E4T_LOG_LAUNCH("adamw8_kernel|n%lld grid%d|%.0f|0", (long long)n, grid, bytes);
    hipLaunchKernelGGL(adamw8_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)s, E4T_ADAMW8_ARGS);
    E4T_CHECK_LAUNCH("adamw8_kernel");
  }
#undef E4T_ADAMW8_ARGS
  return 0;
}
extern "C" int e4t_adamw_rank_ema(float* p, float* m, float* v, float* ema, const void* G, const void* Z, int n, int rows, int cols, int K, int ldg,
                                  long long ldz, float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, float ema_w,
                                  const float* hyper_dev, e4t_stream s) {
  E4T_REQUIRE(p && m && v && ema && G && Z && n > 0 && rows > 0 && cols > 0 && K > 0 && (hyper_dev || step >= 1), "adamw_rank_ema: bad arguments");
  E4T_REQUIRE(cols % 4 == 0 && ldz % 4 == 0 && ldg >= rows && ldz >= (long long)n * cols, "adamw_rank_ema: cols and the Z row stride must be multiples of 4");
  E4T_REQUIRE((((uintptr_t)p | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0 && ((uintptr_t)Z & 7) == 0 && ((uintptr_t)hyper_dev & 15) == 0,
              "adamw_rank_ema: buffers must be 16-B (factors 8-B) aligned");
  const float bc1 = hyper_dev ? 1.f : 1.f - powf(beta1, (float)step), bc2 = hyper_dev ? 1.f : sqrtf(1.f - powf(beta2, (float)step));
  constexpr int RB = 8;
  const int threads = min(320, (cols / 4 + 63) / 64 * 64);
  E4T_LOG_LAUNCH("adamw_rank_ema_kernel<%d>|n%d rows%d cols%d K%d|%.0f|%.0f", RB, n, rows, cols, K, 32.0 * n * rows * cols, 2.0 * n * rows * (double)cols * K);
  hipLaunchKernelGGL((adamw_rank_ema_kernel<RB>), dim3(cdiv(rows, RB), n), dim3(threads), 0, (hipStream_t)s, p, m, v, ema, (const bf16_t*)G, (const bf16_t*)Z, rows,
                     cols, K, ldg, ldz, hyper_dev ? 0.f : lr, beta1, beta2, eps, weight_decay, bc1, bc2, hyper_dev ? 1.f : grad_scale, hyper_dev ? 0.f : ema_w,
                     hyper_dev);
  E4T_CHECK_LAUNCH("adamw_rank_ema_kernel");
  return 0;
}
extern "C" int e4t_ema_update(float* ema, const float* p, long long n, float ema_w, const float* w_dev, e4t_stream s) {
  E4T_REQUIRE(ema && p && n > 0, "ema_update: bad arguments");
  E4T_REQUIRE((((uintptr_t)ema | (uintptr_t)p) & 15) == 0 && ((uintptr_t)w_dev & 3) == 0, "ema_update: buffers must be 16-B aligned");
  E4T_LOG_LAUNCH("ema_update_kernel|n%lld|%.0f|0", (long long)n, 12.0 * (double)n);
  hipLaunchKernelGGL(ema_update_kernel, dim3(grid_for((n + 3) / 4, 4096)), dim3(256), 0, (hipStream_t)s, ema, p, n, w_dev ? 0.f : ema_w, w_dev);
  E4T_CHECK_LAUNCH("ema_update_kernel");
  return 0;
}
extern "C" int e4t_sumsq_partial(const float* g, long long n, float* partial, int nblocks, e4t_stream s) {
  E4T_REQUIRE(g && partial && n > 0 && nblocks > 0, "sumsq_partial: bad arguments");
  hipLaunchKernelGGL(sumsq_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)s, g, n, partial);
  E4T_CHECK_LAUNCH("sumsq_kernel");
  return 0;
}

// ---- in-place row softmax (VAE mid-block attention scores; fp32 math, one 256-thread block per row) ----
namespace {
__global__ __launch_bounds__(256) void softmax_rows_kernel(bf16_t* x, int L, int ld) {
  __shared__ float red[16];
  bf16_t* row = x + (long long)blockIdx.x * ld;
  const int nch = L >> 3;
  float v[8][8];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = threadIdx.x + i * 256;
    if (c < nch) {
      unpack8(*(const uint4*)(row + c * 8), v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) mx = fmaxf(mx, v[i][j]);
    }
  }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = threadIdx.x + i * 256;
    if (c < nch)
#pragma unroll
      for (int j = 0; j < 8; ++j) { v[i][j] = __expf(v[i][j] - mx); s += v[i][j]; }
  }
  s = block_sum(s, red + 8);
  const float inv = 1.f / s;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = threadIdx.x + i * 256;
    if (c < nch) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] *= inv;
      *(uint4*)(row + c * 8) = pack8(v[i]);
    }
  }
}

__global__ __launch_bounds__(256) void im2col3_kernel(const float* px, bf16_t* out, int Bn, int H, int W) {
  const long long total = (long long)Bn * H * W;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % W); long long t = i / W; const int y = (int)(t % H); const int b = (int)(t / H);
    float f[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) f[k] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int yy = y + ky - 1, xx = x + kx - 1;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W)
#pragma unroll
          for (int c = 0; c < 3; ++c) f[(ky * 3 + kx) * 3 + c] = px[(((long long)b * 3 + c) * H + yy) * W + xx];
      }
#pragma unroll
    for (int k = 0; k < 4; ++k) *(uint4*)(out + i * 32 + k * 8) = pack8(f + k * 8);
  }
}
}  // namespace

extern "C" int e4t_softmax_rows(void* x, long long rows, int L, int ld, e4t_stream s) {
  E4T_REQUIRE(x && rows > 0 && L > 0 && L % 8 == 0 && L <= 16384 && ld >= L && ld % 8 == 0, "softmax_rows: bad arguments");
  E4T_REQUIRE(rows <= 0x7fffffffLL, "softmax_rows: too many rows");
  hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)s, (bf16_t*)x, L, ld);
  E4T_CHECK_LAUNCH("softmax_rows_kernel");
  return 0;
}
extern "C" int e4t_im2col3_rgb(const float* pixels_nchw, void* out, int Bn, int H, int W, e4t_stream s) {
  E4T_REQUIRE(pixels_nchw && out && Bn > 0 && H > 0 && W > 0, "im2col3_rgb: bad arguments");
  long long blocks = ((long long)Bn * H * W + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(im2col3_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, pixels_nchw, (bf16_t*)out, Bn, H, W);
  E4T_CHECK_LAUNCH("im2col3_kernel");
  return 0;
}

// ---- im2col-transpose for 3x3 conv weight gradients (tuning mode: every UNet conv weight trains) ----
// out[(tap*C + c)][m] = X[b][iy][ix][c] (zero outside), m = (b, oy, ox) over the conv's OUTPUT pixels, row stride ldo.
// With dY^T this turns dW[co][tap][ci] = sum_m dY[m][co] * X[src(m,tap)][ci] into one NT GEMM whose contraction
// runs over the pixels.  mode: E4T_CONV_S1 / _S2 / _UP2 (same gather rules as the forward conv).
namespace {
__global__ __launch_bounds__(256) void im2col_T_kernel(const bf16_t* x, bf16_t* out, int Hin, int Win, int C, int Hout, int Wout,
                                                       long long Mpix, int ldo, int mode) {
  __shared__ bf16_t tile[64][66];
  const int tap = blockIdx.z, ky = tap / 3, kx = tap - ky * 3;
  const long long m0 = (long long)blockIdx.y * 64;
  const int c0 = blockIdx.x * 64;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rl = ty * 4 + k;
    const long long m = m0 + rl;
    bool ok = m < Mpix;
    long long src = 0;
    if (ok) {
      const int hw = Hout * Wout;
      const int b = (int)(m / hw);
      const int rem = (int)(m - (long long)b * hw);
      const int oy = rem / Wout, ox = rem - oy * Wout;
      int iy, ix;
      if (mode == E4T_CONV_S1) { iy = oy + ky - 1; ix = ox + kx - 1; ok = iy >= 0 && iy < Hin && ix >= 0 && ix < Win; }
      else if (mode == E4T_CONV_S2) { iy = 2 * oy + ky - 1; ix = 2 * ox + kx - 1; ok = iy >= 0 && iy < Hin && ix >= 0 && ix < Win; }
      else { iy = oy + ky - 1; ix = ox + kx - 1; ok = iy >= 0 && iy < 2 * Hin && ix >= 0 && ix < 2 * Win; iy >>= 1; ix >>= 1; }
      src = (((long long)b * Hin + iy) * Win + ix) * C;
    }
    const int c = c0 + tx * 4;
    uint2 v = make_uint2(0, 0);
    if (ok && c < C) v = *(const uint2*)(x + src + c);      // C % 4 == 0
    tile[rl][tx * 4 + 0] = (bf16_t)(v.x & 0xffff); tile[rl][tx * 4 + 1] = (bf16_t)(v.x >> 16);
    tile[rl][tx * 4 + 2] = (bf16_t)(v.y & 0xffff); tile[rl][tx * 4 + 3] = (bf16_t)(v.y >> 16);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int cl = ty * 4 + k, c = c0 + cl;
    const long long m = m0 + tx * 4;
    if (c < C && m < ldo) {                                   // ldo % 4 == 0; columns in [Mpix, ldo) receive the zero fill
      uint2 o;
      o.x = (uint32_t)tile[tx * 4 + 0][cl] | ((uint32_t)tile[tx * 4 + 1][cl] << 16);
      o.y = (uint32_t)tile[tx * 4 + 2][cl] | ((uint32_t)tile[tx * 4 + 3][cl] << 16);
      *(uint2*)(out + ((long long)tap * C + c) * ldo + m) = o;
    }
  }
}
}  // namespace

// ---- plain im2col for the same weight gradients through the TN GEMM (no transposes at all): out[m][tap*C + c] ----
namespace {
__global__ __launch_bounds__(256) void im2col_kernel(const bf16_t* x, bf16_t* out, int Hin, int Win, int C, int Hout, int Wout,
                                                     long long Mpix, int mode) {
  const int cpr = C >> 3;                                     // 16-byte chunks per (pixel, tap)
  const long long total = Mpix * 9 * cpr;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int ch = (int)(idx % cpr);
    const long long t = idx / cpr;
    const int tap = (int)(t % 9);
    const long long m = t / 9;
    const int ky = tap / 3, kx = tap - ky * 3;
    const int hw = Hout * Wout;
    const int b = (int)(m / hw);
    const int rem = (int)(m - (long long)b * hw);
    const int oy = rem / Wout, ox = rem - oy * Wout;
    int iy, ix;
    bool ok;
    if (mode == E4T_CONV_S1) { iy = oy + ky - 1; ix = ox + kx - 1; ok = iy >= 0 && iy < Hin && ix >= 0 && ix < Win; }
    else if (mode == E4T_CONV_S2) { iy = 2 * oy + ky - 1; ix = 2 * ox + kx - 1; ok = iy >= 0 && iy < Hin && ix >= 0 && ix < Win; }
    else { iy = oy + ky - 1; ix = ox + kx - 1; ok = iy >= 0 && iy < 2 * Hin && ix >= 0 && ix < 2 * Win; iy >>= 1; ix >>= 1; }
    uint4 v = make_uint4(0, 0, 0, 0);
    if (ok) v = *(const uint4*)(x + (((long long)b * Hin + iy) * Win + ix) * C + ch * 8);
    *(uint4*)(out + (m * 9 + tap) * C + ch * 8) = v;
  }
}
}  // namespace

extern "C" int e4t_im2col(const void* x, void* out, int Bn, int Hin, int Win, int C, int Hout, int Wout, int mode, e4t_stream s) {
  E4T_REQUIRE(x && out && Bn > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0 && C % 8 == 0, "im2col: bad arguments (C must be a multiple of 8)");
  E4T_REQUIRE(mode == E4T_CONV_S1 || mode == E4T_CONV_S2 || mode == E4T_CONV_UP2, "im2col: mode must be S1, S2 or UP2");
  const long long Mpix = (long long)Bn * Hout * Wout;
  long long blocks = (Mpix * 9 * (C / 8) + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(im2col_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, (const bf16_t*)x, (bf16_t*)out, Hin, Win, C, Hout, Wout,
                     Mpix, mode);
  E4T_CHECK_LAUNCH("im2col_kernel");
  return 0;
}

extern "C" int e4t_im2col_T(const void* x, void* out, int Bn, int Hin, int Win, int C, int Hout, int Wout, int ldo, int mode, e4t_stream s) {
  E4T_REQUIRE(x && out && Bn > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0, "im2col_T: bad arguments");
  E4T_REQUIRE(C > 0 && C % 4 == 0 && ldo % 4 == 0 && (long long)ldo >= (long long)Bn * Hout * Wout, "im2col_T: C, ldo must be multiples of 4, C > 0, ldo >= B*Hout*Wout");
  E4T_REQUIRE(mode == E4T_CONV_S1 || mode == E4T_CONV_S2 || mode == E4T_CONV_UP2, "im2col_T: mode must be S1, S2 or UP2");
  const long long Mpix = (long long)Bn * Hout * Wout;
  hipLaunchKernelGGL(im2col_T_kernel, dim3(cdiv(C, 64), (unsigned)((ldo + 63) / 64), 9), dim3(256), 0, (hipStream_t)s, (const bf16_t*)x, (bf16_t*)out,
                     Hin, Win, C, Hout, Wout, Mpix, ldo, mode);
  E4T_CHECK_LAUNCH("im2col_T_kernel");
  return 0;
}

// ---- masked diffusion loss (the reference's README.md:112-115 TODO on the loss of pretrain_e4t.py:645-647) ----
// loss = sum_{b,c,p} w[b][p] * d^2 / den,  d = pred - target,  den = C * max(sum(w), 1);  dpred = g * 2 * w * d / den.
// Two-stage reductions in a fixed order (per-thread pixel stride, block_sum, then one block over the partials): no atomics, so a
// result is bitwise the same from run to run.  Forward = partial + final, backward = one streaming pass over the saved w * d.
namespace {
constexpr int MMSE_MAX_BLOCKS = 1024;

// one thread per pixel (b, p), all C channels: w is read once, sum(w) falls out of the same pass.  wd (pred's layout, may be null) = w * d.
// WEIGHTED (e4t_weighted_mse_fwd): w may be null (all ones) and the pixel's weight on d is lam[b] * w (lam may be null: all ones), while
// sum(w) — the normaliser — stays the mask's alone; wd = lam * w * d.  WEIGHTED = false is the masked loss, operation for operation.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void masked_mse_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ w,
                                                                 const float* __restrict__ lam, float* __restrict__ wd, float* __restrict__ partial,
                                                                 int B, int C, int HW, int nhwc) {
  __shared__ float red[32];
  const long long npix = (long long)B * HW;
  float se = 0.f, sw = 0.f;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < npix; q += (long long)gridDim.x * 256) {
    const long long b = q / HW;
    const int p = (int)(q - b * HW);
    float wq = (WEIGHTED && !w) ? 1.f : w[q];
    sw += wq;
    if (WEIGHTED && lam) wq = lam[b] * wq;
    for (int c = 0; c < C; ++c) {
      const long long it = (b * C + c) * HW + p;
      const long long ip = nhwc ? q * C + c : it;
      const float d = pred[ip] - target[it];
      const float v = wq * d;
      if (wd) wd[ip] = v;
      se = fmaf(v, d, se);
    }
  }
  se = block_sum(se, red);
  sw = block_sum(sw, red + 16);
  if (threadIdx.x == 0) { partial[blockIdx.x] = se; partial[gridDim.x + blockIdx.x] = sw; }
}
// out[0] = loss, out[1] = den
__global__ __launch_bounds__(256) void masked_mse_final_kernel(const float* __restrict__ partial, int nb, int C, float* __restrict__ out) {
  __shared__ float red[32];
  float se = 0.f, sw = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) { se += partial[i]; sw += partial[nb + i]; }
  se = block_sum(se, red);
  sw = block_sum(sw, red + 16);
  if (threadIdx.x == 0) {
    const float den = (float)C * fmaxf(sw, 1.f);
    out[0] = se / den;
    out[1] = den;
  }
}
__global__ __launch_bounds__(256) void masked_mse_bwd_kernel(const float* __restrict__ wd, const float* __restrict__ stats, const float* __restrict__ g,
                                                             float* __restrict__ dpred, long long n) {
  const float k = g[0] * 2.f / stats[1];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dpred[i] = k * wd[i];
}

// The scheduled pseudo-Huber / smooth-L1 loss (e4t_robust_loss_fwd): masked_mse_partial_kernel<true>'s sibling, the same
// pixel walk and the same two partial rows, so masked_mse_final_kernel finishes it.  Per image c = ctab[t] (t = timesteps[b] clamped into
// the table as diffuse_kernel clamps it; timesteps null = ctab[0]) and, with r = sqrt(d^2 + c^2), h = d^2 / (r + c) — which is r - c
// without the cancellation that costs the textbook form up to 2e-2 at c = 1e3 —
//   huber (kind 1): l = 2 c h, dl/dd = 2 c d / r;   smooth_l1 (kind 2): l = 2 h, dl/dd = 2 d / r.
// With kh = k / 2 = c | 1 the row sums 2 * lam * w * kh * h and wd = lam * w * kh * d / r, half the gradient's numerator, which is what
// masked_mse_bwd_kernel (g * 2 / den * wd) expects.  sqrtf and `/` are the IEEE ones; d == 0 gives h = 0 and wd = 0 as c > 0.
__global__ __launch_bounds__(256) void robust_loss_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ w,
                                                                  const float* __restrict__ lam, const float* __restrict__ ctab,
                                                                  const long long* __restrict__ timesteps, float* __restrict__ wd,
                                                                  float* __restrict__ partial, int B, int C, int HW, int T, int kind, int nhwc) {
  __shared__ float red[32];
  const long long npix = (long long)B * HW;
  float se = 0.f, sw = 0.f;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < npix; q += (long long)gridDim.x * 256) {
    const long long b = q / HW;
    const int p = (int)(q - b * HW);
    long long t = timesteps ? timesteps[b] : 0;
    t = t < 0 ? 0 : (t > T - 1 ? T - 1 : t);
    const float cb = ctab[t], c2 = cb * cb;
    float wq = w ? w[q] : 1.f;
    sw += wq;
    if (lam) wq = lam[b] * wq;
    if (kind == 1) wq = wq * cb;                              // lam * w * k / 2
    const float wq2 = 2.f * wq;
    for (int c = 0; c < C; ++c) {
      const long long it = (b * C + c) * HW + p;
      const long long ip = nhwc ? q * C + c : it;
      const float d = pred[ip] - target[it];
      const float d2 = d * d;
      const float r = sqrtf(d2 + c2);
      if (wd) wd[ip] = wq * d / r;
      se = fmaf(wq2, d2 / (r + cb), se);
    }
  }
  se = block_sum(se, red);
  sw = block_sum(sw, red + 16);
  if (threadIdx.x == 0) { partial[blockIdx.x] = se; partial[gridDim.x + blockIdx.x] = sw; }
}
}  // namespace

extern "C" int e4t_masked_mse_fwd(const float* pred, const float* target, const float* w, float* wd, float* stats, int B, int C, int HW, int pred_nhwc,
                                  e4t_stream s) {
  static_assert(E4T_MASKED_MSE_STATS == 2 + 2 * MMSE_MAX_BLOCKS, "stats = {loss, den} + the two partial rows");
  E4T_REQUIRE(pred && target && w && stats && B > 0 && C > 0 && HW > 0, "masked_mse_fwd: bad arguments");
  const int nb = (int)min(cdivl((long long)B * HW, 256), (long long)MMSE_MAX_BLOCKS);
  hipLaunchKernelGGL(masked_mse_partial_kernel<false>, dim3(nb), dim3(256), 0, (hipStream_t)s, pred, target, w, (const float*)nullptr, wd, stats + 2, B, C,
                     HW, pred_nhwc);
  E4T_CHECK_LAUNCH("masked_mse_partial_kernel");
  hipLaunchKernelGGL(masked_mse_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, (const float*)(stats + 2), nb, C, stats);
  E4T_CHECK_LAUNCH("masked_mse_final_kernel");
  return 0;
}
// the same two launches with a per-image weight lam[B] and an optional mask (min-SNR weighting); the backward is
// e4t_masked_mse_bwd on the saved lam * w * d, whose arithmetic (g * 2 / den * wd) is already the weighted gradient's
extern "C" int e4t_weighted_mse_fwd(const float* pred, const float* target, const float* w, const float* lam, float* wd, float* stats, int B, int C,
                                    int HW, int pred_nhwc, e4t_stream s) {
  E4T_REQUIRE(pred && target && stats && B > 0 && C > 0 && HW > 0, "weighted_mse_fwd: bad arguments (pred, target, stats non-null; B, C, HW > 0)");
  const int nb = (int)min(cdivl((long long)B * HW, 256), (long long)MMSE_MAX_BLOCKS);
  hipLaunchKernelGGL(masked_mse_partial_kernel<true>, dim3(nb), dim3(256), 0, (hipStream_t)s, pred, target, w, lam, wd, stats + 2, B, C, HW, pred_nhwc);
  E4T_CHECK_LAUNCH("weighted_mse_partial_kernel");
  hipLaunchKernelGGL(masked_mse_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, (const float*)(stats + 2), nb, C, stats);
  E4T_CHECK_LAUNCH("masked_mse_final_kernel");
  return 0;
}
// the scheduled pseudo-Huber / smooth-L1 loss in the same two launches; the backward is e4t_masked_mse_bwd on the saved
// lam * w * (k / 2) * d / r, as for the weighted loss
extern "C" int e4t_robust_loss_fwd(const float* pred, const float* target, const float* w, const float* lam, const float* ctab, const long long* timesteps,
                                   float* wd, float* stats, int B, int C, int HW, int T, int kind, int pred_nhwc, e4t_stream s) {
  E4T_REQUIRE(pred && target && ctab && stats && B > 0 && C > 0 && HW > 0,
              "robust_loss_fwd: bad arguments (pred, target, ctab, stats non-null; B, C, HW > 0)");
  E4T_REQUIRE(T >= 1, "robust_loss_fwd: T = %d, the table needs at least one entry", T);
  E4T_REQUIRE(kind == E4T_LOSS_HUBER || kind == E4T_LOSS_SMOOTH_L1, "robust_loss_fwd: kind = %d must be 1 (huber) or 2 (smooth_l1)", kind);
  const int nb = (int)min(cdivl((long long)B * HW, 256), (long long)MMSE_MAX_BLOCKS);
  hipLaunchKernelGGL(robust_loss_partial_kernel, dim3(nb), dim3(256), 0, (hipStream_t)s, pred, target, w, lam, ctab, timesteps, wd, stats + 2, B, C, HW, T,
                     kind, pred_nhwc);
  E4T_CHECK_LAUNCH("robust_loss_partial_kernel");
  hipLaunchKernelGGL(masked_mse_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, (const float*)(stats + 2), nb, C, stats);
  E4T_CHECK_LAUNCH("masked_mse_final_kernel");
  return 0;
}
extern "C" int e4t_masked_mse_bwd(const float* wd, const float* stats, const float* g, float* dpred, long long n, e4t_stream s) {
  E4T_REQUIRE(wd && stats && g && dpred && n > 0, "masked_mse_bwd: bad arguments");
  hipLaunchKernelGGL(masked_mse_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)s, wd, stats, g, dpred, n);
  E4T_CHECK_LAUNCH("masked_mse_bwd_kernel");
  return 0;
}

// ---- the diffusion objective's inputs in one pass (trainer.py add_noise + the target lines) ----
//   n' = noise + s * z[b][c]  (only with an offset: z null = n' is noise itself),  noisy = a*x0 + sg*n',
//   target = n' (epsilon) | a*n' - sg*x0 (v-prediction),  lam[b] = coef[t][2],  {a, sg} = coef[t][0..1],  t = timesteps[b] clamped to the table.
// Every product, sum and difference is rounded on its own, in the order of the torch expressions, so the outputs are those of the stock
// elementwise ops bit for bit.  hipcc's __fmul_rn / __fadd_rn / __fsub_rn are plain `*`, `+`, `-`, which this file's -ffp-contract=fast
// contracts into an FMA like any other (the float4 kernel came out as v_pk_fma_f32: up to 120 ulp from torch where the two products
// cancel), and under that flag `#pragma clang fp contract(off)` is ignored.  So every product goes through mul_rn: the canonicalize
// behind the multiply is dropped at instruction selection (a product is canonical already, it costs no instruction) but leaves the
// combiner no multiply next to the sum or difference to fuse with.  Every sum / difference here has such products as its operands.
// V = 4: HW % 4 == 0 and 16-byte aligned tensors, a float4 never crosses a (b, c) row; V = 1 otherwise.
namespace {
__device__ __forceinline__ float mul_rn(float a, float b) { return __builtin_canonicalizef(a * b); }
__device__ __forceinline__ void diffuse_f(float x, float nz, bool offs, float off, float a, float sg, int vpred, float& ny, float& tg) {
  const float n1 = offs ? nz + off : nz;                     // off = mul_rn(s, z)
  ny = mul_rn(a, x) + mul_rn(sg, n1);
  tg = vpred ? mul_rn(a, n1) - mul_rn(sg, x) : n1;
}
template <int V>
__global__ __launch_bounds__(256) void diffuse_kernel(const float* __restrict__ x0, const float* __restrict__ noise, const float* __restrict__ z,
                                                      const long long* __restrict__ timesteps, const float* __restrict__ coef, float* __restrict__ noisy,
                                                      float* __restrict__ target, float* __restrict__ lam, int B, int C, int HW, int T, float s, int vpred) {
  const int rowg = HW / V;                                   // groups of V elements per (b, c) row
  const long long ng = (long long)B * C * rowg;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < ng; i += (long long)gridDim.x * 256) {
    const long long r = i / rowg;                            // row b * C + c
    const int b = (int)(r / C);
    long long t = timesteps[b];
    t = t < 0 ? 0 : (t > T - 1 ? T - 1 : t);
    const float a = coef[3 * t], sg = coef[3 * t + 1];
    if (i == (long long)b * C * rowg) lam[b] = coef[3 * t + 2];
    const bool offs = z != nullptr;
    const float off = offs ? mul_rn(s, z[r]) : 0.f;
    if (V == 4) {
      const float4 X = *(const float4*)(x0 + i * 4), N = *(const float4*)(noise + i * 4);
      float4 Y, G;
      diffuse_f(X.x, N.x, offs, off, a, sg, vpred, Y.x, G.x);
      diffuse_f(X.y, N.y, offs, off, a, sg, vpred, Y.y, G.y);
      diffuse_f(X.z, N.z, offs, off, a, sg, vpred, Y.z, G.z);
      diffuse_f(X.w, N.w, offs, off, a, sg, vpred, Y.w, G.w);
      *(float4*)(noisy + i * 4) = Y;
      *(float4*)(target + i * 4) = G;
    } else {
      float y, g;
      diffuse_f(x0[i], noise[i], offs, off, a, sg, vpred, y, g);
      noisy[i] = y;
      target[i] = g;
    }
  }
}
}  // namespace

extern "C" int e4t_diffuse(const float* x0, const float* noise, const float* z, const long long* timesteps, const float* coef, float* noisy, float* target,
                           float* lam, int B, int C, int HW, int T, float s, int v_prediction, e4t_stream st) {
  E4T_REQUIRE(x0 && noise && timesteps && coef && noisy && target && lam, "diffuse: null pointer (only z may be null)");
  E4T_REQUIRE(B > 0 && C > 0 && HW > 0 && T > 0, "diffuse: B = %d, C = %d, HW = %d, T = %d must be positive", B, C, HW, T);
  E4T_REQUIRE(z || s == 0.f, "diffuse: a noise offset s = %g needs z", (double)s);
  E4T_REQUIRE(s >= 0.f, "diffuse: the noise offset s = %g must be >= 0", (double)s);
  if (s == 0.f) z = nullptr;                                 // no offset term at all: n' is noise itself, not noise + 0 * z
  const long long n = (long long)B * C * HW;
  const bool vec = HW % 4 == 0 && (((uintptr_t)x0 | (uintptr_t)noise | (uintptr_t)noisy | (uintptr_t)target) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(diffuse_kernel<4>, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)st, x0, noise, z, timesteps, coef, noisy, target, lam, B, C, HW,
                       T, s, v_prediction);
  else
    hipLaunchKernelGGL(diffuse_kernel<1>, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)st, x0, noise, z, timesteps, coef, noisy, target, lam, B, C, HW, T, s,
                       v_prediction);
  E4T_CHECK_LAUNCH("diffuse_kernel");
  return 0;
}
