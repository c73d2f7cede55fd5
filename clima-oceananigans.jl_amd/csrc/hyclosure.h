// hyclosure.h -- the explicit horizontal closures of the HydrostaticFreeSurfaceModel, included by splitexplicit.hip after HyMetric and
// hy_div (it shares their definitions and the no-contraction rule of that file's kernels).
//
//   reference (paths relative to the reference's src/)                                          here
//   TurbulenceClosures/turbulence_closure_implementations/scalar_diffusivity.jl:101              HorizontalScalarDiffusivity(nu, kappa)
//   .../abstract_scalar_diffusivity_closure.jl:179-182, 205-206  (fluxes)                        k_hy_clo_uv<LAP>, k_hy_clo_c<LAP>
//   .../scalar_biharmonic_diffusivity.jl:21                                                       HorizontalScalarBiharmonicDiffusivity
//   .../abstract_scalar_biharmonic_diffusivity_closure.jl:46-50, 66-67, 75-116                    k_hy_clo_uv<BIH>, k_hy_clo_c<BIH>
//   Operators/laplacian_operators.jl:5-18, divergence_operators.jl:35-37, vorticity_operators.jl:2-5
//   TurbulenceClosures/closure_kernel_operators.jl:22-47 (the divergences; their z part is zero here)
//
// Both closures are the last non-zero term of G (hydrostatic_free_surface_tendency_kernel_functions.jl:42-47, 79-84, 116-117), so a
// pass after the advection kernels, G <- G - (a + b) with a the Laplacian's and b the biharmonic's term, leaves the reference's bits:
// a tuple of closures sums its terms in tuple order (closure_tuples.jl:24-55), the vertically implicit closure adds exact zeros with
// no-flux top and bottom, and the sum of two terms does not depend on their order.
//
// One thread per cell (i, j, k), 64-wide rows of threads (the per-row metrics are wave-uniform), every neighbour read from the parent
// arrays: the 2-D stencils of a level stay in the L1 / L2 caches, and there is no vertical coupling.  Every operator keeps the
// reference's operand order; a quotient by a per-row spacing goes through its correctly rounded reciprocal (hy_div) where the grid
// holds one, and `1 / X * (...)` of the reference is a reciprocal times the sum, as written.
//
// Masks (biharmonic only; abstract_scalar_biharmonic_diffusivity_closure.jl:110-116, Grids/inactive_node.jl:60-117): a cell is
// inactive outside the interior of every Bounded direction; a Face-x node (i, j) is peripheral when cell i or i - 1 is inactive, a
// Face-y node when cell j or j - 1 is.  Rows are tested with their GLOBAL index (jrow0 + j), so a latitude band masks what the whole
// grid masks.
struct HyClo {
  int xb, yb, jrow0, gNy;   // Bounded x / y; global row of the band's first row; global row count
};

// the vertical flux divergence of a ConvectiveAdjustmentVerticalDiffusivity in the same pass (hyconvect.h), VZ of the kernels below:
// 0 none (the instances without it), 1 the explicit form (-nu d_z u, -nu d_z v, -kappa d_z c), 2 the implicit form's interior-face
// w-shear of u and v (-nu d_x w, -nu d_y w; the boundary faces keep the explicit flux).  A tuple sums its closures' terms in tuple
// order: o[0..2] list the Laplacian (0), biharmonic (1) and convective-adjustment (2) terms in that order, absent terms are zero.
// VZ 3 and 4 are 1 and 2 with (Center, Center, Center) coefficients (RiBasedVerticalDiffusivity(coefficient_z_location = Center()),
// hyribased.h): kappa at face K is 0.5 (kappa[K-1] + kappa[K]), nu 0.5 (nu_x[K-1] + nu_x[K]) with nu_x the x (or y) interpolation
// (closure_kernel_operators.jl:84-92, the z interpolation of the x one); the third term is then that closure's.
struct HyCvTerm {
  const double* K;         // nu (u, v) or kappa (tracers), (Center, Center, Face); (Center, Center, Center) for VZ 3, 4
  const double* w;         // VZ == 2, 4
  long syk, szk, syw, szw;
  int o0, o1, o2;
};
__device__ inline double hy_cv_sum(const HyCvTerm& z, double l, double b, double v) {
  OCN_NO_CONTRACT
  auto pick = [&](int o) { return o == 0 ? l : o == 1 ? b : v; };
  return (pick(z.o0) + pick(z.o1)) + pick(z.o2);
}

struct HyCloAt {
  // one cell: reference indices (I, J) of the thread's cell, 1-based, J global
  const HyMetric& g;
  const HyClo& m;
  int I, Jg;
  __device__ bool inactive(int di, int dj) const {
    const int a = I + di, b = Jg + dj;
    return (m.xb && (a < 1 || a > g.Nx)) || (m.yb && (b < 1 || b > m.gNy));
  }
  __device__ bool mask_x(int di, int dj) const { return inactive(di, dj) || inactive(di - 1, dj); }   // peripheral_node(Face, Center, Center)
  __device__ bool mask_y(int di, int dj) const { return inactive(di, dj) || inactive(di, dj - 1); }   // peripheral_node(Center, Face, Center)
};

// G_u, G_v -= closure terms at the cell (i, j, k).  LAP: HorizontalScalarDiffusivity(nu); BIH: HorizontalScalarBiharmonicDiffusivity(nu4)
template <bool LAP, bool BIH, int VZ = 0>
__global__ void __launch_bounds__(256) k_hy_clo_uv(HyMetric g, HyClo m, double nu, double nu4, const double* __restrict__ u,
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
    // div_xy^ccc and zeta_3^ffc at (i + di, j + dj)
    auto delta = [&](int di, int dj) {
      return g.r_azcc[r + dj] * ((g.dyfc[r + dj] * U(di + 1, dj) - g.dyfc[r + dj] * U(di, dj)) +
                                 (g.dxcf[r + dj + 1] * V(di, dj + 1) - g.dxcf[r + dj] * V(di, dj)));
    };
    auto zeta = [&](int di, int dj) {
      const double circ = (g.dycf[r + dj] * V(di, dj) - g.dycf[r + dj] * V(di - 1, dj)) -
                          (g.dxfc[r + dj] * U(di, dj) - g.dxfc[r + dj - 1] * U(di, dj - 1));
      return hy_div(circ, g.azff[r + dj], g.r_azff[r + dj]);
    };
    const double d00 = delta(0, 0), z00 = zeta(0, 0);
    // flux_ux = -nu delta, flux_uy = +nu zeta; flux_vx = -nu zeta, flux_vy = -nu delta
    const double fx0 = (g.dyfc[r] * dz) * (-(nu * delta(-1, 0))), fx1 = (g.dyfc[r] * dz) * (-(nu * d00));          // Ax^ccc at i - 1, i
    const double fy0 = (g.dxcf[r] * dz) * (nu * z00), fy1 = (g.dxcf[r + 1] * dz) * (nu * zeta(0, 1));              // Ay^ffc at j, j + 1
    Tu = rVfc * ((fx1 - fx0) + (fy1 - fy0));
    const double gx0 = (g.dycf[r] * dz) * (-(nu * z00)), gx1 = (g.dycf[r] * dz) * (-(nu * zeta(1, 0)));             // Ax^ffc at i, i + 1
    const double gy0 = (g.dxfc[r - 1] * dz) * (-(nu * delta(0, -1))), gy1 = (g.dxfc[r] * dz) * (-(nu * d00));       // Ay^ccc at j - 1, j
    Tv = rVcf * ((gx1 - gx0) + (gy1 - gy0));
  }
  if (BIH) {
    const HyCloAt at{g, m, i + 1, m.jrow0 + j + 1};
    // the masked component Laplacians nabla^2_h^fcc u and nabla^2_h^cfc v at (i + di, j + dj)
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
    const double u00 = Lu(0, 0), um0 = Lu(-1, 0), up0 = Lu(1, 0), u0m = Lu(0, -1), u0p = Lu(0, 1), upm = Lu(1, -1);
    const double v00 = Lv(0, 0), v0p = Lv(0, 1), vm0 = Lv(-1, 0), vmp = Lv(-1, 1), v0m = Lv(0, -1), vp0 = Lv(1, 0);
    // delta* at (i + di, j + dj) from Lu(di, dj), Lu(di + 1, dj), Lv(di, dj), Lv(di, dj + 1); zeta* from Lv(di - 1, dj), Lv(di, dj),
    // Lu(di, dj - 1), Lu(di, dj)
    auto dstar = [&](int dj, double lu0, double lu1, double lv0, double lv1) {
      const int q = r + dj;
      return g.r_azcc[q] * ((g.dyfc[q] * lu1 - g.dyfc[q] * lu0) + (g.dxcf[q + 1] * lv1 - g.dxcf[q] * lv0));
    };
    auto zstar = [&](int dj, double lv0, double lv1, double lu0, double lu1) {
      const int q = r + dj;
      return g.r_azff[q] * ((g.dycf[q] * lv1 - g.dycf[q] * lv0) - (g.dxfc[q] * lu1 - g.dxfc[q - 1] * lu0));
    };
    const double ds00 = dstar(0, u00, up0, v00, v0p), dsm0 = dstar(0, um0, u00, vm0, vmp), ds0m = dstar(-1, u0m, upm, v0m, v00);
    const double zs00 = zstar(0, vm0, v00, u0m, u00), zs01 = zstar(1, vmp, v0p, u00, u0p), zs10 = zstar(0, v00, vp0, upm, up0);
    // flux_ux = +nu4 delta*, flux_uy = -nu4 zeta*; flux_vx = +nu4 zeta*, flux_vy = +nu4 delta*
    const double fx0 = (g.dyfc[r] * dz) * (nu4 * dsm0), fx1 = (g.dyfc[r] * dz) * (nu4 * ds00);
    const double fy0 = (g.dxcf[r] * dz) * (-(nu4 * zs00)), fy1 = (g.dxcf[r + 1] * dz) * (-(nu4 * zs01));
    const double bu = rVfc * ((fx1 - fx0) + (fy1 - fy0));
    const double gx0 = (g.dycf[r] * dz) * (nu4 * zs00), gx1 = (g.dycf[r] * dz) * (nu4 * zs10);
    const double gy0 = (g.dxfc[r - 1] * dz) * (nu4 * ds0m), gy1 = (g.dxfc[r] * dz) * (nu4 * ds00);
    const double bv = rVcf * ((gx1 - gx0) + (gy1 - gy0));
    if (VZ) {
      bu_ = bu;
      bv_ = bv;
    } else {
      Tu = LAP ? Tu + bu : bu;
      Tv = LAP ? Tv + bv : bv;
    }
  }
  if (VZ) {
    // faces k + 1 (K) and k + 2 (K + 1) of this cell; nu at the velocity points 0.5 (nu[i-1] + nu[i]) / 0.5 (nu[j-1] + nu[j])
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

// G_c -= closure terms for NT tracers at the cell (i, j, k); kap[t] the Laplacian, kap4[t] the biharmonic diffusivity of tracer t
template <bool LAP, bool BIH, int NT, int VZ = 0>
__global__ void __launch_bounds__(256) k_hy_clo_c(HyMetric g, HyClo m, double kap0, double kap1, double kap40, double kap41,
                                                  const double* __restrict__ c0, const double* __restrict__ c1, double* __restrict__ G0,
                                                  double* __restrict__ G1, long syc, long szc, HyCvTerm z) {
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
      const double kap = t ? kap1 : kap0;
      // flux = -kappa d c
      const double fx0 = ax * ((-kap) * dxc(0, 0)), fx1 = ax * ((-kap) * dxc(1, 0));
      const double fy0 = ay0 * ((-kap) * dyc(0, 0)), fy1 = ay1 * ((-kap) * dyc(0, 1));
      T = rV * ((fx1 - fx0) + (fy1 - fy0));
    }
    if (BIH) {
      const double kap4 = t ? kap41 : kap40;
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
      const double b = rV * ((ax * (kap4 * sx1) - ax * (kap4 * sx0)) + (ay1 * (kap4 * sy1) - ay0 * (kap4 * sy0)));
      if (VZ) b_ = b;
      else T = LAP ? T + b : b;
    }
    if (VZ) {
      // -kappa d_z c at faces k + 1 and k + 2 of this cell (kappa as it is: one kappa serves every tracer)
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
