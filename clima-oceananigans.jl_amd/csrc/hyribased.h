// hyribased.h -- RiBasedVerticalDiffusivity (RBVD) of the HydrostaticFreeSurfaceModel, included by splitexplicit.hip after hyconvect.h
// (it shares HyGrid, HyBuoy, hy_cv_dzb and the no-contraction rule of that file's kernels).
//
//   reference (paths relative to the reference's src/)                                          here
//   TurbulenceClosures/turbulence_closure_implementations/ri_based_vertical_diffusivity.jl:57-154
//                                                                                                k_hy_ri_diff (in update_state!), hy_ri_taper
//   .../CATKEVerticalDiffusivities/mixing_length.jl:174-180 (Ri at (Center, Center, Face))      k_hy_ri_diff
//   closure_kernel_operators.jl:84-101, Operators/interpolation_operators.jl:63-67               HyCvCol<3..5>, k_hy_clo_*<.., 3 / 4>
//
// Diffusivities.  kappa = kappa0 taper(Ri, Ri0kappa, Ridkappa), nu = nu0 taper(Ri, Ri0nu, Ridnu), with
//   Ri = ifelse(N^2 == 0, 0, N^2 / (d_z u^2 + d_z v^2)),  d_z u^2 = 0.5 ((d_z u)^2[i] + (d_z u)^2[i+1]),  d_z v^2 alike along y,
// every term at face k.  The division is an IEEE division on purpose: N^2 != 0 over zero shear gives +-Inf, which every taper maps to
// exactly 0 (Ri = +Inf) or exactly 1 (Ri = -Inf).  The reference picks Ri with `ifelse(LZ === Type{Face}, Ri_ccc, Ri_ccf)`; LZ is
// Face or Center itself, never Type{Face}, so the test is always false and Ri is Ri_ccf at face k for BOTH locations: with
// coefficient_z_location = Center() the cell-centred kappa[i, j, k] holds the value of face k.  Ported as written.
//
// The reference launches over :xyz, so faces (or centres) 1..Nz of the grid's columns get a value; fill_halo_regions! then fills x / y
// like any Center field and, for a Center location only, the first halo level on either side in z (no-flux).  Face Nz + 1 and the z
// halos of a Face location stay zero.  Here one thread per interior column marches up the column with the vertical neighbours of
// u, v, T and S in registers, and the library's own fills (hfield_fill, with the band exchange) do the rest.  At face 1 the halo
// level 0 of u, v, T and S is a zero-gradient copy, so N^2 = 0, Ri = 0 and kappa = kappa0 taper(0): the Face-location solve never
// reads face 1, the Center-location one reaches it through the z interpolation at face 2.
struct HyRiParam {
  double nu0, Ri0nu, Ridnu, k0, Ri0k, Ridk;
};

// taper(Ri, x0, d): TAPER 0 PiecewiseLinear, 1 Exponential, 2 HyperbolicTangent (ri_based_vertical_diffusivity.jl:131-133)
template <int TAPER>
__device__ inline double hy_ri_taper(double x, double x0, double d) {
  OCN_NO_CONTRACT
  const double y = (x - x0) / d;
  if (TAPER == 0) return 1.0 - fmin(1.0, fmax(0.0, y));
  if (TAPER == 1) return exp(-fmax(0.0, y));
  return (1.0 - tanh(y)) / 2;
}

// kappa, nu at k = 1..Nz of the interior columns (faces for a Face location, centres for Center: the same values, the strides of the
// coefficient fields differ).  u: (Face, Center, Center), v: (Center, Face, Center), T / S: tracers or null
template <int TAPER>
__global__ void k_hy_ri_diff(HyGrid g, HyBuoy q, HyRiParam p, const double* __restrict__ u, const double* __restrict__ v,
                             const double* __restrict__ T, const double* __restrict__ S, double* __restrict__ kap, double* __restrict__ nu,
                             long syu, long szu, long syv, long szv, long sy, long sz, long syk, long szk) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= g.Nx || j >= g.Ny) return;
  const long x = i + g.Hx, y = j + g.Hy;
  long cu = x + y * syu + (long)(g.Hz - 1) * szu, cv = x + y * syv + (long)(g.Hz - 1) * szv, c = x + y * sy + (long)(g.Hz - 1) * sz;
  long ck = x + y * syk + (long)g.Hz * szk;
  // level 0 (the halo below level 1)
  double u0 = u[cu], u1 = u[cu + 1], v0 = v[cv], v1 = v[cv + syv], tl = T ? T[c] : 0.0, sl = S ? S[c] : 0.0;
  for (int k = 0; k < g.Nz; ++k, ck += szk) {
    cu += szu;
    cv += szv;
    c += sz;
    const double uh0 = u[cu], uh1 = u[cu + 1], vh0 = v[cv], vh1 = v[cv + syv], th = T ? T[c] : 0.0, sh = S ? S[c] : 0.0;
    const double dzf = g.dzf[k];
    const double du0 = (uh0 - u0) / dzf, du1 = (uh1 - u1) / dzf, dv0 = (vh0 - v0) / dzf, dv1 = (vh1 - v1) / dzf;
    const double su = 0.5 * (du0 * du0 + du1 * du1), sv = 0.5 * (dv0 * dv0 + dv1 * dv1);
    const double N2 = hy_cv_dzb(q, tl, th, sl, sh, dzf);
    const double Ri = N2 == 0 ? 0.0 : N2 / (su + sv);
    kap[ck] = p.k0 * hy_ri_taper<TAPER>(Ri, p.Ri0k, p.Ridk);
    nu[ck] = p.nu0 * hy_ri_taper<TAPER>(Ri, p.Ri0nu, p.Ridnu);
    u0 = uh0;
    u1 = uh1;
    v0 = vh0;
    v1 = vh1;
    tl = th;
    sl = sh;
  }
}
