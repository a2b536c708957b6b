// Body of adamw_rank_kernel<RB> / adamw_rank_ema_kernel<RB> (optim.hip), included once into each, as adamw_kernel.inc is: the plain kernel keeps
// its symbol and its code.  EMA: the average of the stack moves in the same pass (32 B per parameter); hyper is then float[8], [4] = w.
  if (hyper) { lr = hyper[0]; bc1 = hyper[1]; bc2_sqrt = hyper[2]; gscale = hyper[3]; if constexpr (EMA) ema_w = hyper[4]; }
  __shared__ float gs[16 * RB];                      // G[k0 + k][r0 + rr] as fp32, [rr][k]
  const int slot = blockIdx.y, r0 = blockIdx.x * RB;
  const int Q = cols >> 2;
  for (int q = threadIdx.x; q < (Q + (int)blockDim.x - 1) / (int)blockDim.x * (int)blockDim.x; q += blockDim.x) {      // (uniform trip count: barriers inside)
    const bool on = q < Q;
    float acc[RB][4];
#pragma unroll
    for (int rr = 0; rr < RB; ++rr)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[rr][j] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 16) {
      __syncthreads();
      for (int i = threadIdx.x; i < 16 * RB; i += blockDim.x) {
        const int rr = i >> 4, k = i & 15;
        gs[i] = (k0 + k < K && r0 + rr < rows) ? bf2f(G[(long long)(k0 + k) * ldg + r0 + rr]) : 0.f;
      }
      float z[16][4];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        uint2 w = make_uint2(0u, 0u);
        if (on && k0 + k < K) w = *(const uint2*)(Z + (long long)(k0 + k) * ldz + (long long)slot * cols + 4 * q);
        unpack4(w, z[k]);
      }
      __syncthreads();
#pragma unroll
      for (int rr = 0; rr < RB; ++rr) {
        const float4* g4 = (const float4*)(gs + rr * 16);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const float4 g = g4[kk];                   // broadcast read
          const float gk[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[rr][j] = fmaf(gk[u], z[kk * 4 + u][j], acc[rr][j]);
        }
      }
    }
    if (!on) continue;
#pragma unroll
    for (int rr = 0; rr < RB; ++rr) {
      if (r0 + rr >= rows) continue;
      const long long i = ((long long)slot * rows + r0 + rr) * cols + 4 * q;
      float4 P = *(float4*)(p + i), M = *(float4*)(m + i), V = *(float4*)(v + i);
      float pp[4] = {P.x, P.y, P.z, P.w}, mm[4] = {M.x, M.y, M.z, M.w}, vv[4] = {V.x, V.y, V.z, V.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gg = acc[rr][j] * gscale;
        pp[j] *= 1.f - lr * wd;
        mm[j] = b1 * mm[j] + (1.f - b1) * gg;
        vv[j] = b2 * vv[j] + (1.f - b2) * gg * gg;
        const float denom = sqrtf(vv[j]) / bc2_sqrt + eps;
        pp[j] -= (lr / bc1) * mm[j] / denom;
      }
      *(float4*)(p + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
      *(float4*)(m + i) = make_float4(mm[0], mm[1], mm[2], mm[3]);
      *(float4*)(v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
      if constexpr (EMA) {
        const float4 E = *(float4*)(ema + i);
        *(float4*)(ema + i) = make_float4(ema_f(E.x, pp[0], ema_w), ema_f(E.y, pp[1], ema_w), ema_f(E.z, pp[2], ema_w), ema_f(E.w, pp[3], ema_w));
      }
    }
  }
