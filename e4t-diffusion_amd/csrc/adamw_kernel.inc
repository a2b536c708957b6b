// Body of adamw_kernel / adamw_ema_kernel (optim.hip), included once into each: the two __global__ kernels differ only in what they bind to
// EMA, ema and ema_w, so the plain kernel keeps its symbol and, not being routed through a shared device function, its code (DESIGN §2.1, §2.3c).
// EMA: the average `ema` of the weights moves in the same pass, e' = ema_f(e, p', w) with p' the value this thread stores; hyper is then float[8], [4] = w.
  if (hyper) { lr = hyper[0]; bc1 = hyper[1]; bc2_sqrt = hyper[2]; gscale = hyper[3]; if constexpr (EMA) ema_w = hyper[4]; }
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * 1024) {
    if (i + 4 <= n) {
      float4 P = *(float4*)(p + i), M = *(float4*)(m + i), V = *(float4*)(v + i);
      const float4 G = *(const float4*)(g + i);
      float pp[4] = {P.x, P.y, P.z, P.w}, mm[4] = {M.x, M.y, M.z, M.w}, vv[4] = {V.x, V.y, V.z, V.w};
      const float gg[4] = {G.x * gscale, G.y * gscale, G.z * gscale, G.w * gscale};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        pp[k] *= 1.f - lr * wd;
        mm[k] = b1 * mm[k] + (1.f - b1) * gg[k];
        vv[k] = b2 * vv[k] + (1.f - b2) * gg[k] * gg[k];
        const float denom = sqrtf(vv[k]) / bc2_sqrt + eps;
        pp[k] -= (lr / bc1) * mm[k] / denom;
      }
      *(float4*)(p + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
      *(float4*)(m + i) = make_float4(mm[0], mm[1], mm[2], mm[3]);
      *(float4*)(v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
      if constexpr (EMA) {
        const float4 E = *(float4*)(ema + i);
        *(float4*)(ema + i) = make_float4(ema_f(E.x, pp[0], ema_w), ema_f(E.y, pp[1], ema_w), ema_f(E.z, pp[2], ema_w), ema_f(E.w, pp[3], ema_w));
      }
    } else {
      for (long long j = i; j < n; ++j) {
        float pp = p[j] * (1.f - lr * wd);
        const float gg = g[j] * gscale;
        const float mm = b1 * m[j] + (1.f - b1) * gg, vv = b2 * v[j] + (1.f - b2) * gg * gg;
        pp -= (lr / bc1) * mm / (sqrtf(vv) / bc2_sqrt + eps);
        p[j] = pp; m[j] = mm; v[j] = vv;
        if constexpr (EMA) ema[j] = ema_f(ema[j], pp, ema_w);
      }
    }
  }
