// hyclosure_var.h -- the explicit horizontal closures with coefficients that follow the grid, and the HorizontalDivergence
// formulations; included by splitexplicit.hip after hyclosure.h, whose kernels these restate with two differences and nothing else
// (same thread layout, operand order, masks and no-contraction rule; the constant-coefficient instances of hyclosure.h stay as they are
// and serve every closure these differences do not touch).
//
//   reference (paths relative to the reference's src/)                                          here
//   TurbulenceClosures/closure_kernel_operators.jl:72-125 (nu^ccc, nu^ffc, kappa^fcc, kappa^cfc)   HyCoef, hy_coef
//   .../discrete_diffusion_function.jl:69-73, turbulence_closure_utils.jl:3-25                    the host evaluates the function once
//   .../abstract_scalar_diffusivity_closure.jl:194-196  (HorizontalDivergenceFormulation)         div2: flux_ux = flux_vy = -nu delta
//   .../abstract_scalar_biharmonic_diffusivity_closure.jl:56-57                                   div4: flux_ux = flux_vy = +nu delta*
//
// A coefficient is zonally uniform: regular x on both grids, so a grid-scaled coefficient or a function of (y, z) / (phi, z) does not
// depend on i.  Here it is two (row, level) tables, one per location the reference evaluates it at:
//   nu     a at (Center, Center, Center) for the delta / delta* fluxes,   b at (Face, Face, Center) for the zeta / zeta* fluxes
//   kappa  a at (Face, Center, Center) for the x flux,                    b at (Center, Face, Center) for the y flux
// Entry [r + k * rows]: r the row of the per-row metric arrays (row j - 1 + Hy of the grid or band, halo rows included, rows =
// Ny + 2 Hy + 1), k = 0 .. Nz - 1 the level.  Rows and levels are wave-uniform in these kernels (one row per wave, k = blockIdx.z), so
// a table read is a scalar load next to the metrics' and costs no vector register.  A number that shares a launch with a table or with
// a divergence formulation comes as a constant table (the host keeps one per value): one accessor, no second path in the kernels.
struct HyCoef {
  const double* a;
  const double* b;
};
__device__ inline double hy_coef(const double* tab, int rows, int r, int k) { return tab[r + (long)k * rows]; }

// G_u, G_v -= closure terms at the cell (i, j, k): k_hy_clo_uv with nu2 / nu4 through hy_coef; DIV2 / DIV4 choose the
// HorizontalDivergence formulation of the Laplacian / biharmonic term: the zeta (zeta*) fluxes are the zero fallback and nothing that
// only they need -- zeta, zeta*, Lu(0, 1), Lv(1, 0) -- is evaluated
template <bool LAP, bool BIH, int VZ, bool DIV2, bool DIV4>
__global__ void __launch_bounds__(256) k_hy_clo_uv_var(HyMetric g, HyClo m, HyCoef n2, HyCoef n4, int rows, const double* __restrict__ u,
                                                       const double* __restrict__ v, double* __restrict__ Gu, double* __restrict__ Gv, long syu,
                                                       long szu, long syv, long szv, HyCvTerm z) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y, k = blockIdx.z;
  if (i >= g.Nx || j >= g.Ny) return;
  const int r = OCN_UNIFORM(j + g.Hy);       // blockDim.x == 64: one row per wave
  const long cu = (i + g.Hx) + (long)r * syu + (long)(k + g.Hz) * szu, cv = (i + g.Hx) + (long)r * syv + (long)(k + g.Hz) * szv;
  auto U = [&](int di, int dj) { return u[cu + di + dj * syu]; };
  auto V = [&](int di, int dj) { return v[cv + di + dj * syv]; };
  const double dz = g.dzc[k];
  const double rVfc = 1 / (g.azcc[r] * dz), rVcf = 1 / (g.azff[r] * dz);      // 1 / V^fcc (Az^fc = Az^cc), 1 / V^cfc (Az^cf = Az^ff)
  double Tu = 0.0, Tv = 0.0, bu_ = 0.0, bv_ = 0.0;
  if (LAP) {
    auto delta = [&](int di, int dj) {
      return g.r_azcc[r + dj] * ((g.dyfc[r + dj] * U(di + 1, dj) - g.dyfc[r + dj] * U(di, dj)) +
                                 (g.dxcf[r + dj + 1] * V(di, dj + 1) - g.dxcf[r + dj] * V(di, dj)));
    };
    auto zeta = [&](int di, int dj) {
      const double circ = (g.dycf[r + dj] * V(di, dj) - g.dycf[r + dj] * V(di - 1, dj)) -
                          (g.dxfc[r + dj] * U(di, dj) - g.dxfc[r + dj - 1] * U(di, dj - 1));
      return hy_div(circ, g.azff[r + dj], g.r_azff[r + dj]);
    };
    const double nc = hy_coef(n2.a, rows, r, k), ncs = hy_coef(n2.a, rows, r - 1, k);       // nu^ccc at rows j, j - 1
    const double d00 = delta(0, 0);
    // flux_ux = -nu delta, flux_vy = -nu delta
    const double fx0 = (g.dyfc[r] * dz) * (-(nc * delta(-1, 0))), fx1 = (g.dyfc[r] * dz) * (-(nc * d00));          // Ax^ccc at i - 1, i
    const double gy0 = (g.dxfc[r - 1] * dz) * (-(ncs * delta(0, -1))), gy1 = (g.dxfc[r] * dz) * (-(nc * d00));     // Ay^ccc at j - 1, j
    if (DIV2) {
      Tu = rVfc * ((fx1 - fx0) + 0.0);
      Tv = rVcf * (0.0 + (gy1 - gy0));
    } else {
      const double nf = hy_coef(n2.b, rows, r, k), nfn = hy_coef(n2.b, rows, r + 1, k);     // nu^ffc at rows j, j + 1
      const double z00 = zeta(0, 0);
      // flux_uy = +nu zeta; flux_vx = -nu zeta
      const double fy0 = (g.dxcf[r] * dz) * (nf * z00), fy1 = (g.dxcf[r + 1] * dz) * (nfn * zeta(0, 1));            // Ay^ffc at j, j + 1
      Tu = rVfc * ((fx1 - fx0) + (fy1 - fy0));
      const double gx0 = (g.dycf[r] * dz) * (-(nf * z00)), gx1 = (g.dycf[r] * dz) * (-(nf * zeta(1, 0)));           // Ax^ffc at i, i + 1
      Tv = rVcf * ((gx1 - gx0) + (gy1 - gy0));
    }
  }
  if (BIH) {
    const HyCloAt at{g, m, i + 1, m.jrow0 + j + 1};
    auto Lu = [&](int di, int dj) {
      const int q = r + dj;
      auto ax = [&](int e) { return (g.dyfc[q] * dz) * hy_div(U(e + 1, dj) - U(e, dj), g.dxfc[q], g.r_dxfc[q]); };     // Ax d_x^ccc u at i + e
      auto ay = [&](int e) { return (g.dxcf[q + e] * dz) * hy_div(U(di, dj + e) - U(di, dj + e - 1), g.dycf[q + e], g.r_dycf[q + e]); };   // Ay d_y^ffc u
      const double L = (1 / (g.azcc[q] * dz)) * ((ax(di) - ax(di - 1)) + (ay(1) - ay(0)));
      return at.mask_x(di, dj) ? 0.0 : L;
    };
    auto Lv = [&](int di, int dj) {
      const int q = r + dj;
      auto ax = [&](int e) { return (g.dycf[q] * dz) * ((V(e, dj) - V(e - 1, dj)) / g.dxcf[q]); };                      // Ax d_x^ffc v at i + e
      auto ay = [&](int e) { return (g.dxfc[q + e] * dz) * ((V(di, dj + e + 1) - V(di, dj + e)) / g.dyfc[q + e]); };   // Ay d_y^ccc v at j + e
      const double L = (1 / (g.azff[q] * dz)) * ((ax(di + 1) - ax(di)) + (ay(0) - ay(-1)));
      return at.mask_y(di, dj) ? 0.0 : L;
    };
    const double u00 = Lu(0, 0), um0 = Lu(-1, 0), up0 = Lu(1, 0), u0m = Lu(0, -1), u0p = DIV4 ? 0.0 : Lu(0, 1), upm = Lu(1, -1);
    const double v00 = Lv(0, 0), v0p = Lv(0, 1), vm0 = Lv(-1, 0), vmp = Lv(-1, 1), v0m = Lv(0, -1), vp0 = DIV4 ? 0.0 : Lv(1, 0);
    auto dstar = [&](int dj, double lu0, double lu1, double lv0, double lv1) {
      const int q = r + dj;
      return g.r_azcc[q] * ((g.dyfc[q] * lu1 - g.dyfc[q] * lu0) + (g.dxcf[q + 1] * lv1 - g.dxcf[q] * lv0));
    };
    auto zstar = [&](int dj, double lv0, double lv1, double lu0, double lu1) {
      const int q = r + dj;
      return g.r_azff[q] * ((g.dycf[q] * lv1 - g.dycf[q] * lv0) - (g.dxfc[q] * lu1 - g.dxfc[q - 1] * lu0));
    };
    const double nc = hy_coef(n4.a, rows, r, k), ncs = hy_coef(n4.a, rows, r - 1, k);       // nu^ccc at rows j, j - 1
    const double ds00 = dstar(0, u00, up0, v00, v0p), dsm0 = dstar(0, um0, u00, vm0, vmp), ds0m = dstar(-1, u0m, upm, v0m, v00);
    // flux_ux = +nu4 delta*, flux_vy = +nu4 delta*
    const double fx0 = (g.dyfc[r] * dz) * (nc * dsm0), fx1 = (g.dyfc[r] * dz) * (nc * ds00);
    const double gy0 = (g.dxfc[r - 1] * dz) * (ncs * ds0m), gy1 = (g.dxfc[r] * dz) * (nc * ds00);
    double bu, bv;
    if (DIV4) {
      bu = rVfc * ((fx1 - fx0) + 0.0);
      bv = rVcf * (0.0 + (gy1 - gy0));
    } else {
      const double nf = hy_coef(n4.b, rows, r, k), nfn = hy_coef(n4.b, rows, r + 1, k);     // nu^ffc at rows j, j + 1
      const double zs00 = zstar(0, vm0, v00, u0m, u00), zs01 = zstar(1, vmp, v0p, u00, u0p), zs10 = zstar(0, v00, vp0, upm, up0);
      // flux_uy = -nu4 zeta*; flux_vx = +nu4 zeta*
      const double fy0 = (g.dxcf[r] * dz) * (-(nf * zs00)), fy1 = (g.dxcf[r + 1] * dz) * (-(nfn * zs01));
      bu = rVfc * ((fx1 - fx0) + (fy1 - fy0));
      const double gx0 = (g.dycf[r] * dz) * (nf * zs00), gx1 = (g.dycf[r] * dz) * (nf * zs10);
      bv = rVcf * ((gx1 - gx0) + (gy1 - gy0));
    }
    if (VZ) {
      bu_ = bu;
      bv_ = bv;
    } else {
      Tu = LAP ? Tu + bu : bu;
      Tv = LAP ? Tv + bv : bv;
    }
  }
  if (VZ) {
    // as in k_hy_clo_uv: faces k + 1 (K) and k + 2 (K + 1) of this cell
    const int Nz = g.Nz;
    const long ck = (i + g.Hx) + (long)r * z.syk + (long)(k + g.Hz) * z.szk;
    const double azu = g.azcc[r], azv = g.azff[r];          // Az^fcf = Az^cc, Az^cff = Az^ff
    auto flux = [&](int e, bool isv) {                       // the flux at face K + e
      const long q = ck + (long)e * z.szk;
      double nf;
      if (VZ >= 3) {         // centres K - 1 (q - szk) and K (q)
        const long d = isv ? z.syk : 1;
        nf = 0.5 * (0.5 * (z.K[q - z.szk - d] + z.K[q - z.szk]) + 0.5 * (z.K[q - d] + z.K[q]));
      } else {
        nf = isv ? 0.5 * (z.K[q - z.syk] + z.K[q]) : 0.5 * (z.K[q - 1] + z.K[q]);
      }
      const int K = k + 1 + e;
      if ((VZ == 2 || VZ == 4) && K > 1 && K < Nz + 1) {
        const long cw = (i + g.Hx) + (long)r * z.syw + (long)(K - 1 + g.Hz) * z.szw;
        return isv ? -nf * ((z.w[cw] - z.w[cw - z.syw]) / g.dycf[r]) : -nf * ((z.w[cw] - z.w[cw - 1]) / g.dxfc[r]);
      }
      const long c = (isv ? cv : cu) + (long)e * (isv ? szv : szu);
      const double* f = isv ? v : u;
      return -nf * ((f[c] - f[c - (isv ? szv : szu)]) / g.dzf[K - 1]);
    };
    const double zu = rVfc * (azu * flux(1, false) - azu * flux(0, false));
    const double zv = rVcf * (azv * flux(1, true) - azv * flux(0, true));
    Tu = hy_cv_sum(z, LAP ? Tu : 0.0, bu_, zu);
    Tv = hy_cv_sum(z, LAP ? Tv : 0.0, bv_, zv);
  }
  Gu[cu] = Gu[cu] - Tu;
  Gv[cv] = Gv[cv] - Tv;
}

// G_c -= closure terms for NT tracers at the cell (i, j, k): k_hy_clo_c with kappa through hy_coef (k2[t] the Laplacian, k4[t] the
// biharmonic diffusivity of tracer t): kappa^fcc of row j on both x fluxes, kappa^cfc of rows j and j + 1 on the y fluxes
struct HyCoef2 { HyCoef t[2]; };
template <bool LAP, bool BIH, int NT, int VZ = 0>
__global__ void __launch_bounds__(256) k_hy_clo_c_var(HyMetric g, HyClo m, HyCoef2 k2, HyCoef2 k4, int rows, const double* __restrict__ c0,
                                                      const double* __restrict__ c1, double* __restrict__ G0, double* __restrict__ G1, long syc,
                                                      long szc, HyCvTerm z) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y, k = blockIdx.z;
  if (i >= g.Nx || j >= g.Ny) return;
  const int r = OCN_UNIFORM(j + g.Hy);       // blockDim.x == 64: one row per wave
  const long cc = (i + g.Hx) + (long)r * syc + (long)(k + g.Hz) * szc;
  const double dz = g.dzc[k];
  const double rV = 1 / (g.azcc[r] * dz);
  const double ax = g.dyfc[r] * dz, ay0 = g.dxcf[r] * dz, ay1 = g.dxcf[r + 1] * dz;      // Ax^fcc, Ay^cfc at j, j + 1
  const HyCloAt at{g, m, i + 1, m.jrow0 + j + 1};
  const bool mx0 = BIH && at.mask_x(0, 0), mx1 = BIH && at.mask_x(1, 0), my0 = BIH && at.mask_y(0, 0), my1 = BIH && at.mask_y(0, 1);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const double* c = (t ? c1 : c0) + cc;
    auto C = [&](int di, int dj) { return c[di + dj * syc]; };
    auto dxc = [&](int di, int dj) { const int q = r + dj; return hy_div(C(di, dj) - C(di - 1, dj), g.dxfc[q], g.r_dxfc[q]); };   // d_x^fcc c
    auto dyc = [&](int di, int dj) { const int q = r + dj; return hy_div(C(di, dj) - C(di, dj - 1), g.dycf[q], g.r_dycf[q]); };   // d_y^cfc c
    double T = 0.0, b_ = 0.0;
    if (LAP) {
      const HyCoef& q2 = k2.t[t];
      const double kx = hy_coef(q2.a, rows, r, k), ky0 = hy_coef(q2.b, rows, r, k), ky1 = hy_coef(q2.b, rows, r + 1, k);
      // flux = -kappa d c
      const double fx0 = ax * ((-kx) * dxc(0, 0)), fx1 = ax * ((-kx) * dxc(1, 0));
      const double fy0 = ay0 * ((-ky0) * dyc(0, 0)), fy1 = ay1 * ((-ky1) * dyc(0, 1));
      T = rV * ((fx1 - fx0) + (fy1 - fy0));
    }
    if (BIH) {
      const HyCoef& q4 = k4.t[t];
      const double kx = hy_coef(q4.a, rows, r, k), ky0 = hy_coef(q4.b, rows, r, k), ky1 = hy_coef(q4.b, rows, r + 1, k);
      // nabla^2_h^ccc c at (i + di, j + dj), unmasked
      auto L = [&](int di, int dj) {
        const int q = r + dj;
        return (1 / (g.azcc[q] * dz)) * (((g.dyfc[q] * dz) * dxc(di + 1, dj) - (g.dyfc[q] * dz) * dxc(di, dj)) +
                                         ((g.dxcf[q + 1] * dz) * dyc(di, dj + 1) - (g.dxcf[q] * dz) * dyc(di, dj)));
      };
      const double l00 = L(0, 0), lm0 = L(-1, 0), lp0 = L(1, 0), l0m = L(0, -1), l0p = L(0, 1);
      // flux_x = kappa4 mask_x(1 / Az^fc delta_x(Dy^cc L)), flux_y = kappa4 mask_y(1 / Az^cf delta_y(Dx^cc L))
      const double sx0 = mx0 ? 0.0 : g.r_azcc[r] * (g.dyfc[r] * l00 - g.dyfc[r] * lm0);
      const double sx1 = mx1 ? 0.0 : g.r_azcc[r] * (g.dyfc[r] * lp0 - g.dyfc[r] * l00);
      const double sy0 = my0 ? 0.0 : g.r_azff[r] * (g.dxfc[r] * l00 - g.dxfc[r - 1] * l0m);
      const double sy1 = my1 ? 0.0 : g.r_azff[r + 1] * (g.dxfc[r + 1] * l0p - g.dxfc[r] * l00);
      const double b = rV * ((ax * (kx * sx1) - ax * (kx * sx0)) + (ay1 * (ky1 * sy1) - ay0 * (ky0 * sy0)));
      if (VZ) b_ = b;
      else T = LAP ? T + b : b;
    }
    if (VZ) {
      // -kappa d_z c at faces k + 1 and k + 2 of this cell, as in k_hy_clo_c
      const long ck = (i + g.Hx) + (long)r * z.syk + (long)(k + g.Hz) * z.szk;
      auto kf = [&](long q) { return VZ >= 3 ? 0.5 * (z.K[q - z.szk] + z.K[q]) : z.K[q]; };
      auto flux = [&](int e) { return -kf(ck + (long)e * z.szk) * ((c[(long)e * szc] - c[(long)(e - 1) * szc]) / g.dzf[k + e]); };
      const double az = g.azcc[r];
      T = hy_cv_sum(z, LAP ? T : 0.0, b_, rV * (az * flux(1) - az * flux(0)));
    }
    double* G = (t ? G1 : G0) + cc;
    *G = *G - T;
  }
}

// the launches: what is on picks the instance (VZ as in hyclosure.h; without a vertical term the kernel of no term at all is not
// launched by the caller)
struct HyCloUVArgs {
  HyMetric g; HyClo m; HyCoef n2, n4; int rows;
  const double *u, *v; double *Gu, *Gv; long syu, szu, syv, szv; HyCvTerm z;
};
template <bool LAP, bool BIH, int VZ, bool DIV2, bool DIV4>
static void hy_clo_uv_var_launch(dim3 gr, dim3 b, hipStream_t s, const HyCloUVArgs& a) {
  ocn_launch(k_hy_clo_uv_var<LAP, BIH, VZ, DIV2, DIV4>, gr, b, s, a.g, a.m, a.n2, a.n4, a.rows, a.u, a.v, a.Gu, a.Gv, a.syu, a.szu, a.syv, a.szv, a.z);
}
// the formulations of the terms that are on (a term that is off has no formulation: no instance for it)
template <bool LAP, bool BIH, int VZ>
static void hy_clo_uv_var_forms(bool div2, bool div4, dim3 gr, dim3 b, hipStream_t s, const HyCloUVArgs& a) {
  if constexpr (LAP && BIH) {
    if (div2 && div4) hy_clo_uv_var_launch<true, true, VZ, true, true>(gr, b, s, a);
    else if (div2) hy_clo_uv_var_launch<true, true, VZ, true, false>(gr, b, s, a);
    else if (div4) hy_clo_uv_var_launch<true, true, VZ, false, true>(gr, b, s, a);
    else hy_clo_uv_var_launch<true, true, VZ, false, false>(gr, b, s, a);
  } else if constexpr (LAP) {
    if (div2) hy_clo_uv_var_launch<true, false, VZ, true, false>(gr, b, s, a);
    else hy_clo_uv_var_launch<true, false, VZ, false, false>(gr, b, s, a);
  } else if constexpr (BIH) {
    if (div4) hy_clo_uv_var_launch<false, true, VZ, false, true>(gr, b, s, a);
    else hy_clo_uv_var_launch<false, true, VZ, false, false>(gr, b, s, a);
  } else {
    hy_clo_uv_var_launch<false, false, VZ, false, false>(gr, b, s, a);
  }
}
template <int VZ>
static void hy_clo_uv_var_terms(bool lap, bool bih, bool div2, bool div4, dim3 gr, dim3 b, hipStream_t s, const HyCloUVArgs& a) {
  if (lap && bih) hy_clo_uv_var_forms<true, true, VZ>(div2, div4, gr, b, s, a);
  else if (lap) hy_clo_uv_var_forms<true, false, VZ>(div2, div4, gr, b, s, a);
  else if (bih) hy_clo_uv_var_forms<false, true, VZ>(div2, div4, gr, b, s, a);
  else if constexpr (VZ != 0) hy_clo_uv_var_forms<false, false, VZ>(div2, div4, gr, b, s, a);
}
static void hy_clo_uv_var(int vz, bool lap, bool bih, bool div2, bool div4, dim3 gr, dim3 b, hipStream_t s, const HyCloUVArgs& a) {
  switch (vz) {
    case 0: hy_clo_uv_var_terms<0>(lap, bih, div2, div4, gr, b, s, a); break;
    case 1: hy_clo_uv_var_terms<1>(lap, bih, div2, div4, gr, b, s, a); break;
    case 2: hy_clo_uv_var_terms<2>(lap, bih, div2, div4, gr, b, s, a); break;
    case 3: hy_clo_uv_var_terms<3>(lap, bih, div2, div4, gr, b, s, a); break;
    default: hy_clo_uv_var_terms<4>(lap, bih, div2, div4, gr, b, s, a);
  }
}

struct HyCloCArgs {
  HyMetric g; HyClo m; HyCoef2 k2, k4; int rows;
  const double *c0, *c1; double *G0, *G1; long syc, szc; HyCvTerm z;
};
template <bool LAP, bool BIH, int NT, int VZ>
static void hy_clo_c_var_launch(dim3 gr, dim3 b, hipStream_t s, const HyCloCArgs& a) {
  ocn_launch(k_hy_clo_c_var<LAP, BIH, NT, VZ>, gr, b, s, a.g, a.m, a.k2, a.k4, a.rows, a.c0, a.c1, a.G0, a.G1, a.syc, a.szc, a.z);
}
template <int NT, int VZ>
static void hy_clo_c_var_terms(bool lap, bool bih, dim3 gr, dim3 b, hipStream_t s, const HyCloCArgs& a) {
  if (lap && bih) hy_clo_c_var_launch<true, true, NT, VZ>(gr, b, s, a);
  else if (lap) hy_clo_c_var_launch<true, false, NT, VZ>(gr, b, s, a);
  else if (bih) hy_clo_c_var_launch<false, true, NT, VZ>(gr, b, s, a);
  else if constexpr (VZ != 0) hy_clo_c_var_launch<false, false, NT, VZ>(gr, b, s, a);
}
// vz: 0, 1 or 3 (the tracers have no w-shear form)
static void hy_clo_c_var(int vz, bool two, bool lap, bool bih, dim3 gr, dim3 b, hipStream_t s, const HyCloCArgs& a) {
  if (two) {
    if (vz == 0) hy_clo_c_var_terms<2, 0>(lap, bih, gr, b, s, a);
    else if (vz == 1) hy_clo_c_var_terms<2, 1>(lap, bih, gr, b, s, a);
    else hy_clo_c_var_terms<2, 3>(lap, bih, gr, b, s, a);
  } else {
    if (vz == 0) hy_clo_c_var_terms<1, 0>(lap, bih, gr, b, s, a);
    else if (vz == 1) hy_clo_c_var_terms<1, 1>(lap, bih, gr, b, s, a);
    else hy_clo_c_var_terms<1, 3>(lap, bih, gr, b, s, a);
  }
}
