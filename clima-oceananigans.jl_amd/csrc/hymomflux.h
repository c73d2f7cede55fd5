// hymomflux.h -- flux-form momentum advection of the hydrostatic model on a RectilinearGrid: k_hy_Guv_flux (included from
// splitexplicit.hip after k_hy_Guv, whose Coriolis and pressure-gradient device functions it shares).
//
// Restated from the reference (paths relative to its src/):
//   Advection/vector_invariant_advection.jl:100-101          U_dot_grad_u = div_Uu for every AbstractAdvectionScheme
//   Advection/momentum_advection_operators.jl:52-71          div_Uu at fcc, div_Uv at cfc: 1 / V (d_x Fx + d_y Fy + d_z Fz)
//   Advection/centered_second_order.jl:16-26                 C2: interpolated Ax u, Ay v, Az w times second-order interpolants
//   Advection/centered_advective_fluxes.jl:15-26             C4: area x symmetric advecting velocity x symmetric interpolant
//   Advection/upwind_biased_advective_fluxes.jl:10-100       U1, U3, U5, WENO5: area x upwind_biased_product(u~, q^L, q^R)
//   Advection/topologically_conditional_interpolation.jl:19-83   second order inside the boundary buffer of a Bounded direction
//   Models/HydrostaticFreeSurfaceModels/hydrostatic_free_surface_model.jl:201-210   flux form only where the grid is not curvilinear
//
// One thread per column marching upwards on 64 x 4 blocks, like k_hy_Guv.  The vertical fluxes Wu (Face, Center, Face) and Wv
// (Center, Face, Face) through a level's upper face are kept in registers for the next level, whose lower face it is (same operands,
// same bits).  The horizontal face fluxes are formed by both columns they separate, from the same operands in the same order (as in
// k_hy_Gc_hi) -- nothing crosses lanes.
//
// CenteredSecondOrder keeps the reference's operand order without contraction (bit parity with the NumPy oracle, like k_hy_Gc); the
// higher orders use the reconstructions of stencils.h as they are (fast reciprocal and contraction inside: parity to round-off).
// Halo cells read: 1 for C2 and U1, 2 for C4 and U3, 3 for U5 and WENO5 -- of u, v and, for the four-point advecting velocity, two
// columns / rows of w (w[i-2 .. i+1]); the vector-invariant kernel reads one.
#pragma once

// adv_flux_b of stencils.h, but for UpwindBiasedThirdOrder restated without contraction: recon_low leaves the compiler free to fuse
// 2 p[0] + 5 p[-s] - p[-2s] either way, and it fused two inlined copies of one flux differently (1 ulp apart: a uniform u then left
// G_u = -2e-20 instead of 0).  Uncontracted, the two columns that form a face's flux get the same bits.
template <int ADV>
OCN_DEVFN double hy_flux_b(const double* p, long s, double ut, bool bounded, int idx, int N, int nb) {
  OCN_NO_CONTRACT
  if (ADV != ADV_U3) return adv_flux_b<ADV>(p, s, ut, bounded, idx, N, nb);
  const bool pos = ut > 0.0;
  if (bounded && !(pos ? outside_left(idx, N, nb) : outside_right(idx, N, nb))) return ut * sym2(p - s, s);
  return ut * (pos ? (2.0 * p[0] + 5.0 * p[-s] - p[-2 * s]) / 6.0 : (-p[s] + 5.0 * p[0] + 2.0 * p[-s]) / 6.0);
}

template <int ADV>
__global__ void __launch_bounds__(256) k_hy_Guv_flux(HyMetric g, HyPhys ph, const double* __restrict__ u, const double* __restrict__ v,
                                                     const double* __restrict__ w, const double* __restrict__ p, double* __restrict__ Gu,
                                                     double* __restrict__ Gv, long syu, long szu, long syv, long szv, long syc, long szc) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= g.Nx || j >= g.Ny) return;
  constexpr int NB = (ADV == ADV_U5 || ADV == ADV_WENO_Z) ? 2 : 1;      // boundary_buffer of the scheme (C2 has none)
  const int r = OCN_UNIFORM(j + g.Hy);       // blockDim.x == 64: one row per wave
  long cu = (i + g.Hx) + (long)r * syu + (long)g.Hz * szu, cv = (i + g.Hx) + (long)r * syv + (long)g.Hz * szv;
  long cc = (i + g.Hx) + (long)r * syc + (long)g.Hz * szc;       // w and pHY' share the (Center, Center) row pitch
  const long szw = szc;
  auto U = [&](int di, int dj, int dk) { return u[cu + di + dj * syu + dk * szu]; };
  auto V = [&](int di, int dj, int dk) { return v[cv + di + dj * syv + dk * szv]; };
  auto W = [&](int di, int dj, int dk) { return w[cc + di + dj * syc + dk * szw]; };
  const bool xb = ph.xb != 0, yb = ph.yb != 0;
  const int ig = i + 1, jg = ph.jrow0 + j + 1;          // 1-based (global) indices of the buffer tests
  const double dxfc = g.dxfc[r], dycf = g.dycf[r], rdxfc = g.r_dxfc[r], rdycf = g.r_dycf[r];
  const double dyfc = g.dyfc[r], dyfcm = g.dyfc[r - 1], dxcf = g.dxcf[r], dxcfm = g.dxcf[r - 1], dxcfp = g.dxcf[r + 1], azcc = g.azcc[r];
  // Wu, Wv through the face below level k + dk (0-based level k of the marching pointers; 1-based face index kf)
  auto Wuv = [&](int dk, int kf, double& Wu, double& Wv) {
    if (ADV == ADV_C2) {
      Wu = (0.5 * (azcc * W(-1, 0, dk) + azcc * W(0, 0, dk))) * (0.5 * (U(0, 0, dk - 1) + U(0, 0, dk)));
      Wv = (0.5 * (azcc * W(0, -1, dk) + azcc * W(0, 0, dk))) * (0.5 * (V(0, 0, dk - 1) + V(0, 0, dk)));
    } else {
      const double* wk = w + cc + dk * szw;
      const double wx = sym_b<ADV>(wk - 1, 1, xb, ig, g.Nx, NB), wy = sym_b<ADV>(wk - syc, syc, yb, jg, ph.gNy, NB);
      Wu = azcc * hy_flux_b<ADV>(u + cu + dk * szu, szu, wx, true, kf, g.Nz, NB);
      Wv = azcc * hy_flux_b<ADV>(v + cv + dk * szv, szv, wy, true, kf, g.Nz, NB);
    }
  };
  double Wu_lo, Wv_lo;
  Wuv(0, 1, Wu_lo, Wv_lo);
  for (int k = 0; k < g.Nz; ++k, cu += szu, cv += szv, cc += szc) {
    const double dz = g.dzc[k];
    double Wu_hi, Wv_hi;
    Wuv(1, k + 2, Wu_hi, Wv_hi);
    double Au, Av;
    if (ADV == ADV_C2) {
      const double ax = dyfc * dz, axm = dyfcm * dz, ay = dxcf * dz, aym = dxcfm * dz, ayp = dxcfp * dz;
      // div_Uu: Fx at centres i - 1, i; Fy at (Face, Face) rows j, j + 1
      const double au0 = ax * U(0, 0, 0);
      const double uFx0 = (0.5 * (ax * U(-1, 0, 0) + au0)) * (0.5 * (U(-1, 0, 0) + U(0, 0, 0)));
      const double uFx1 = (0.5 * (au0 + ax * U(1, 0, 0))) * (0.5 * (U(0, 0, 0) + U(1, 0, 0)));
      const double uFy0 = (0.5 * (ay * V(-1, 0, 0) + ay * V(0, 0, 0))) * (0.5 * (U(0, -1, 0) + U(0, 0, 0)));
      const double uFy1 = (0.5 * (ayp * V(-1, 1, 0) + ayp * V(0, 1, 0))) * (0.5 * (U(0, 0, 0) + U(0, 1, 0)));
      Au = 1 / (azcc * dz) * (((uFx1 - uFx0) + (uFy1 - uFy0)) + (Wu_hi - Wu_lo));
      // div_Uv: Fx at (Face, Face) columns i, i + 1; Fy at centres j - 1, j
      const double av0 = ay * V(0, 0, 0);
      const double vFx0 = (0.5 * (axm * U(0, -1, 0) + ax * U(0, 0, 0))) * (0.5 * (V(-1, 0, 0) + V(0, 0, 0)));
      const double vFx1 = (0.5 * (axm * U(1, -1, 0) + ax * U(1, 0, 0))) * (0.5 * (V(0, 0, 0) + V(1, 0, 0)));
      const double vFy0 = (0.5 * (aym * V(0, -1, 0) + av0)) * (0.5 * (V(0, -1, 0) + V(0, 0, 0)));
      const double vFy1 = (0.5 * (av0 + ayp * V(0, 1, 0))) * (0.5 * (V(0, 0, 0) + V(0, 1, 0)));
      Av = 1 / (azcc * dz) * (((vFx1 - vFx0) + (vFy1 - vFy0)) + (Wv_hi - Wv_lo));
    } else {
      const double *uc = u + cu, *vc = v + cv;
      // div_Uu.  Fx at centres i - 1, i: u~ = symmetric interpolation of u to the centre, u reconstructed to it (the face form at the
      // centre's upper face, buffer test with the centre's index); Fy at (Face, Face) rows j, j + 1: v~ = v interpolated along x
      const double ux0 = sym_b<ADV>(uc - 1, 1, xb, ig - 1, g.Nx, NB), ux1 = sym_b<ADV>(uc, 1, xb, ig, g.Nx, NB);
      const double uFx0 = (dyfc * dz) * hy_flux_b<ADV>(uc, 1, ux0, xb, ig - 1, g.Nx, NB);
      const double uFx1 = (dyfc * dz) * hy_flux_b<ADV>(uc + 1, 1, ux1, xb, ig, g.Nx, NB);
      const double vx0 = sym_b<ADV>(vc - 1, 1, xb, ig, g.Nx, NB), vx1 = sym_b<ADV>(vc + syv - 1, 1, xb, ig, g.Nx, NB);
      const double uFy0 = (dxcf * dz) * hy_flux_b<ADV>(uc, syu, vx0, yb, jg, ph.gNy, NB);
      const double uFy1 = (dxcfp * dz) * hy_flux_b<ADV>(uc + syu, syu, vx1, yb, jg + 1, ph.gNy, NB);
      Au = 1 / (azcc * dz) * (((uFx1 - uFx0) + (uFy1 - uFy0)) + (Wu_hi - Wu_lo));
      // div_Uv.  Fx at (Face, Face) columns i, i + 1: u~ = u interpolated along y; Fy at centres j - 1, j
      const double uy0 = sym_b<ADV>(uc - syu, syu, yb, jg, ph.gNy, NB), uy1 = sym_b<ADV>(uc + 1 - syu, syu, yb, jg, ph.gNy, NB);
      const double vFx0 = (dyfc * dz) * hy_flux_b<ADV>(vc, 1, uy0, xb, ig, g.Nx, NB);
      const double vFx1 = (dyfc * dz) * hy_flux_b<ADV>(vc + 1, 1, uy1, xb, ig + 1, g.Nx, NB);
      const double vy0 = sym_b<ADV>(vc - syv, syv, yb, jg - 1, ph.gNy, NB), vy1 = sym_b<ADV>(vc, syv, yb, jg, ph.gNy, NB);
      const double vFy0 = (dxcfm * dz) * hy_flux_b<ADV>(vc, syv, vy0, yb, jg - 1, ph.gNy, NB);
      const double vFy1 = (dxcf * dz) * hy_flux_b<ADV>(vc + syv, syv, vy1, yb, jg, ph.gNy, NB);
      Av = 1 / (azcc * dz) * (((vFx1 - vFx0) + (vFy1 - vFy0)) + (Wv_hi - Wv_lo));
    }
    Wu_lo = Wu_hi;
    Wv_lo = Wv_hi;
    const HyPair C = hy_coriolis_uv(g, ph.cor, ph.f0, ph.frow, r, U, V, dxfc, rdxfc, dycf, rdycf);
    const HyPair gp = hy_pressure_gradient(p + cc, syc, dxfc, rdxfc, dycf, rdycf);
    Gu[cu] = ((-Au - 0.0) - C.u) - gp.u;
    Gv[cv] = ((-Av - 0.0) - C.v) - gp.v;
  }
}

// Flux-form WENO5(grid = grid) on a stretched z: k_hy_Guv_flux<ADV_WENO_Z> with the candidates of the z reconstructions of Wu and Wv
// taken from the row of face k of the table tab (hywenoz.h: hy_flux_sz); every other flux, Coriolis and the pressure gradient are the
// same expressions.  A kernel of its own, so that k_hy_Guv_flux's instantiations keep their code.
__global__ void __launch_bounds__(256) k_hy_Guv_flux_sz(HyMetric g, HyPhys ph, const double* __restrict__ u, const double* __restrict__ v,
                                                        const double* __restrict__ w, const double* __restrict__ p, double* __restrict__ Gu,
                                                        double* __restrict__ Gv, const double* __restrict__ tab, long syu, long szu, long syv,
                                                        long szv, long syc, long szc) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= g.Nx || j >= g.Ny) return;
  constexpr int ADV = ADV_WENO_Z, NB = 2;
  const int r = OCN_UNIFORM(j + g.Hy);       // blockDim.x == 64: one row per wave
  long cu = (i + g.Hx) + (long)r * syu + (long)g.Hz * szu, cv = (i + g.Hx) + (long)r * syv + (long)g.Hz * szv;
  long cc = (i + g.Hx) + (long)r * syc + (long)g.Hz * szc;
  const long szw = szc;
  auto U = [&](int di, int dj, int dk) { return u[cu + di + dj * syu + dk * szu]; };
  auto V = [&](int di, int dj, int dk) { return v[cv + di + dj * syv + dk * szv]; };
  const bool xb = ph.xb != 0, yb = ph.yb != 0;
  const int ig = i + 1, jg = ph.jrow0 + j + 1;
  const double dxfc = g.dxfc[r], dycf = g.dycf[r], rdxfc = g.r_dxfc[r], rdycf = g.r_dycf[r];
  const double dyfc = g.dyfc[r], dxcf = g.dxcf[r], dxcfm = g.dxcf[r - 1], dxcfp = g.dxcf[r + 1], azcc = g.azcc[r];
  // Wu, Wv through the face below level k + dk; kf: the face's 1-based index, the same in every lane (its table row: scalar loads)
  auto Wuv = [&](int dk, int kf, double& Wu, double& Wv) {
    const double* wk = w + cc + dk * szw;
    const double wx = sym_b<ADV>(wk - 1, 1, xb, ig, g.Nx, NB), wy = sym_b<ADV>(wk - syc, syc, yb, jg, ph.gNy, NB);
    const double* tk = tab + 12 * OCN_UNIFORM(kf);
    Wu = azcc * hy_flux_sz(u + cu + dk * szu, szu, wx, kf, g.Nz, tk);
    Wv = azcc * hy_flux_sz(v + cv + dk * szv, szv, wy, kf, g.Nz, tk);
  };
  double Wu_lo, Wv_lo;
  Wuv(0, 1, Wu_lo, Wv_lo);
  for (int k = 0; k < g.Nz; ++k, cu += szu, cv += szv, cc += szc) {
    const double dz = g.dzc[k];
    double Wu_hi, Wv_hi;
    Wuv(1, k + 2, Wu_hi, Wv_hi);
    const double *uc = u + cu, *vc = v + cv;
    const double ux0 = sym_b<ADV>(uc - 1, 1, xb, ig - 1, g.Nx, NB), ux1 = sym_b<ADV>(uc, 1, xb, ig, g.Nx, NB);
    const double uFx0 = (dyfc * dz) * hy_flux_b<ADV>(uc, 1, ux0, xb, ig - 1, g.Nx, NB);
    const double uFx1 = (dyfc * dz) * hy_flux_b<ADV>(uc + 1, 1, ux1, xb, ig, g.Nx, NB);
    const double vx0 = sym_b<ADV>(vc - 1, 1, xb, ig, g.Nx, NB), vx1 = sym_b<ADV>(vc + syv - 1, 1, xb, ig, g.Nx, NB);
    const double uFy0 = (dxcf * dz) * hy_flux_b<ADV>(uc, syu, vx0, yb, jg, ph.gNy, NB);
    const double uFy1 = (dxcfp * dz) * hy_flux_b<ADV>(uc + syu, syu, vx1, yb, jg + 1, ph.gNy, NB);
    const double Au = 1 / (azcc * dz) * (((uFx1 - uFx0) + (uFy1 - uFy0)) + (Wu_hi - Wu_lo));
    const double uy0 = sym_b<ADV>(uc - syu, syu, yb, jg, ph.gNy, NB), uy1 = sym_b<ADV>(uc + 1 - syu, syu, yb, jg, ph.gNy, NB);
    const double vFx0 = (dyfc * dz) * hy_flux_b<ADV>(vc, 1, uy0, xb, ig, g.Nx, NB);
    const double vFx1 = (dyfc * dz) * hy_flux_b<ADV>(vc + 1, 1, uy1, xb, ig + 1, g.Nx, NB);
    const double vy0 = sym_b<ADV>(vc - syv, syv, yb, jg - 1, ph.gNy, NB), vy1 = sym_b<ADV>(vc, syv, yb, jg, ph.gNy, NB);
    const double vFy0 = (dxcfm * dz) * hy_flux_b<ADV>(vc, syv, vy0, yb, jg - 1, ph.gNy, NB);
    const double vFy1 = (dxcf * dz) * hy_flux_b<ADV>(vc + syv, syv, vy1, yb, jg, ph.gNy, NB);
    const double Av = 1 / (azcc * dz) * (((vFx1 - vFx0) + (vFy1 - vFy0)) + (Wv_hi - Wv_lo));
    Wu_lo = Wu_hi;
    Wv_lo = Wv_hi;
    const HyPair C = hy_coriolis_uv(g, ph.cor, ph.f0, ph.frow, r, U, V, dxfc, rdxfc, dycf, rdycf);
    const HyPair gp = hy_pressure_gradient(p + cc, syc, dxfc, rdxfc, dycf, rdycf);
    Gu[cu] = ((-Au - 0.0) - C.u) - gp.u;
    Gv[cv] = ((-Av - 0.0) - C.v) - gp.v;
  }
}
