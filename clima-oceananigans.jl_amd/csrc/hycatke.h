// hycatke.h -- CATKEVerticalDiffusivity of the HydrostaticFreeSurfaceModel, included by splitexplicit.hip after hyribased.h (it shares
// HyGrid, HyBuoy, hy_cv_dzb, HyCvSolve / HyCvCol and the no-contraction rule of that file's kernels).
//
//   reference (paths relative to the reference's src/)                                          here
//   .../CATKEVerticalDiffusivities/CATKEVerticalDiffusivities.jl:155-212 (calculate_CATKE_diffusivities!, Ku / Kc / Ke)
//   .../CATKEVerticalDiffusivities/mixing_length.jl:97-263                                       k_hy_catke_diff (in update_state!)
//   .../CATKEVerticalDiffusivities/turbulent_kinetic_energy_equation.jl:15-49                    k_hy_catke_diff (L^e), k_hy_catke_src
//   Models/HydrostaticFreeSurfaceModels/hydrostatic_free_surface_tendency_kernel_functions.jl:144-169
//                                                                                                k_hy_catke_src (after the tracer pass)
//   TurbulenceClosures/vertically_implicit_diffusion_solver.jl:87-91                             HyCvColLin, k_hy_cv_*_lin
//
// Diffusivities.  One thread per interior column marches up the faces K = 1..Nz + 1 with the level below in registers.  What the
// reference evaluates three or four times per face (in Ku, Kc, Ke and the dissipation coefficient) is evaluated once: the shear
// Ix(d_z u)^2 + Iy(d_z v)^2, N^2, e+ = Iz max(0, e), u* = Iz sqrt(max(0, e)) -- two different interpolations --, Ri and the tanh of
// the stability functions.  Every `ifelse` is a select: the 0 / 0 and x / 0 operands of the branch not taken are computed and dropped.
// The momentum length is sigma_u max(C^delta_u dz, l*) without the convective length, as the reference has it (its max(l^h, ...) line
// is commented out); the tracer and TKE lengths take max(l^h, ...).
//
// K^u, K^c, K^e hold the value of face k at index k = 1..Nz.  The reference's fields are CenterFields with the boundary conditions of
// a (Center, Center, Face) location, and for an auxiliary field those are `nothing` at the bottom and the top of a Bounded z
// (field_boundary_conditions.jl:33, 135-143): nothing is filled in z, index 1 keeps the value the kernel wrote -- shear production and
// buoyancy flux of level 1 read it -- and index Nz + 1, a halo cell of the CenterField that the :xyz launch never reaches, stays zero.
// The mixing length of face Nz + 1 is still evaluated, from the halo level as the reference does, because
// L^e[k] = -C^D sqrt|e[k]| / (0.5 (l_e[k] + l_e[k+1])) reads it; l_e of the face below waits in a register.  dw[K - 1] is the wall
// distance min(z_F[Nz+1] - z_F[K], z_F[K] - z_F[1]) of face K, tabulated by the setter.
struct HyCatkeParam {
  double CD;
  double Cbu, Cbc, Cbe;        // min(C^b, C^b_phi)
  double Csu, Csc, Cse;        // min(C^s, C^s_phi)
  double Cdu, Cdc, Cde;        // C^delta
  double CAc, CAe, CASc, CASe; // the convective lengths of tracers and TKE (the momentum's is computed and dropped by the reference)
  double Ku0, Kur, Kc0, Kcr, Ke0, Ker, Riw, Ric;
};

// the diagonal's implicit linear term of one field: L at the centres of the field's columns
struct HyCvLin {
  const double* L;
  long sy, sz;
};

__device__ inline double hy_catke_pos(double x) { return x > 0.0 ? x : 0.0; }          // max(0, x)

__global__ void k_hy_catke_diff(HyGrid g, HyBuoy q, HyCatkeParam p, const double* __restrict__ dw, const double* __restrict__ Qb,
                                const double* __restrict__ u, const double* __restrict__ v, const double* __restrict__ T,
                                const double* __restrict__ S, const double* __restrict__ e, double* __restrict__ Ku, double* __restrict__ Kc,
                                double* __restrict__ Ke, double* __restrict__ Le, long syu, long szu, long syv, long szv, long sy, long sz,
                                long syk, long szk, long syl, long szl) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= g.Nx || j >= g.Ny) return;
  const long x = i + g.Hx, y = j + g.Hy;
  long cu = x + y * syu + (long)(g.Hz - 1) * szu, cv = x + y * syv + (long)(g.Hz - 1) * szv, c = x + y * sy + (long)(g.Hz - 1) * sz;
  long ck = x + y * syk + (long)g.Hz * szk, cl = x + y * syl + (long)g.Hz * szl;
  const double qb = Qb ? Qb[i + (long)j * g.Nx] : 0.0;
  const double inf = __builtin_inf();
  // level 0 (the halo below level 1)
  double u0 = u[cu], u1 = u[cu + 1], v0 = v[cv], v1 = v[cv + syv], tl = T ? T[c] : 0.0, sl = S ? S[c] : 0.0, el = e[c];
  double lel = 0.0;                          // l_e of the face below
  for (int K = 1; K <= g.Nz + 1; ++K, ck += szk) {
    cu += szu;
    cv += szv;
    c += sz;
    const double uh0 = u[cu], uh1 = u[cu + 1], vh0 = v[cv], vh1 = v[cv + syv], th = T ? T[c] : 0.0, sh = S ? S[c] : 0.0, eh = e[c];
    const double dzf = g.dzf[K - 1];
    const double du0 = (uh0 - u0) / dzf, du1 = (uh1 - u1) / dzf, dv0 = (vh0 - v0) / dzf, dv1 = (vh1 - v1) / dzf;
    const double su = 0.5 * (du0 * du0 + du1 * du1), sv = 0.5 * (dv0 * dv0 + dv1 * dv1);
    const double S2 = su + sv, Sh = sqrt(S2);
    const double N2 = hy_cv_dzb(q, tl, th, sl, sh, dzf);
    const double Np = sqrt(fmax(0.0, N2));
    const double ep = 0.5 * (hy_catke_pos(el) + hy_catke_pos(eh));
    const double us = 0.5 * (sqrt(hy_catke_pos(el)) + sqrt(hy_catke_pos(eh)));
    const double sqe = sqrt(ep);
    const double lb = Np == 0 ? inf : sqe / Np;
    const double ls = Sh == 0 ? inf : sqe / Sh;
    const double Ri = N2 == 0 ? 0.0 : N2 / S2;
    const double step = 1 + tanh((Ri - p.Ric) / p.Riw);
    const double d = dw[K - 1];
    // convective_mixing_length: l^A and alpha are shared, C^A and C^As differ
    const double alpha = Sh * qb / ep;
    const double lA = sqrt(ep * ep * ep) / qb;
    const bool convecting = (N2 < 0) & (qb > 0) & (ep > 0);
    const double lhc = convecting ? p.CAc * lA * (1 - p.CASc * alpha) : 0.0;
    const double lhe = convecting ? p.CAe * lA * (1 - p.CASe * alpha) : 0.0;
    const double lu = (p.Ku0 + p.Kur * step) * fmax(p.Cdu * dzf, fmin(fmin(d, p.Cbu * lb), p.Csu * ls));
    const double lc = fmax(lhc, (p.Kc0 + p.Kcr * step) * fmax(p.Cdc * dzf, fmin(fmin(d, p.Cbc * lb), p.Csc * ls)));
    const double le = fmax(lhe, (p.Ke0 + p.Ker * step) * fmax(p.Cde * dzf, fmin(fmin(d, p.Cbe * lb), p.Cse * ls)));
    if (K <= g.Nz) {
      Ku[ck] = lu * us;
      Kc[ck] = lc * us;
      Ke[ck] = le * us;
    }
    if (K > 1) {
      Le[cl] = -p.CD * sqrt(fabs(el)) / (0.5 * (lel + le));          // centre K - 1
      cl += szl;
    }
    lel = le;
    u0 = uh0;
    u1 = uh1;
    v0 = vh0;
    v1 = vh1;
    tl = th;
    sl = sh;
    el = eh;
  }
}

// the source terms of the TKE tendency: G <- (G + Iz(K^u) (Ixz(d_z u)^2 + Iyz(d_z v)^2)) + (-Iz(K^c) Iz(N^2)) over the grid's cells, after
// the tracer pass (advection and the tuple's explicit terms) and before the flux conditions, the reference's order of the sum.  One
// thread per column, the face below in registers; K^u and K^c hold zero at face Nz + 1
__global__ void k_hy_catke_src(HyGrid g, HyBuoy q, const double* __restrict__ u, const double* __restrict__ v, const double* __restrict__ T,
                               const double* __restrict__ S, const double* __restrict__ Ku, const double* __restrict__ Kc, double* __restrict__ G,
                               long syu, long szu, long syv, long szv, long sy, long sz, long syk, long szk) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= g.Nx || j >= g.Ny) return;
  const long x = i + g.Hx, y = j + g.Hy;
  long cu = x + y * syu + (long)(g.Hz - 1) * szu, cv = x + y * syv + (long)(g.Hz - 1) * szv, c = x + y * sy + (long)(g.Hz - 1) * sz;
  long ck = x + y * syk + (long)g.Hz * szk;
  double u0 = u[cu], u1 = u[cu + 1], v0 = v[cv], v1 = v[cv + syv], tl = T ? T[c] : 0.0, sl = S ? S[c] : 0.0;
  double sul = 0.0, svl = 0.0, n2l = 0.0, kul = 0.0, kcl = 0.0;      // face K - 1
  for (int K = 1; K <= g.Nz + 1; ++K, ck += szk) {
    cu += szu;
    cv += szv;
    c += sz;
    const double uh0 = u[cu], uh1 = u[cu + 1], vh0 = v[cv], vh1 = v[cv + syv], th = T ? T[c] : 0.0, sh = S ? S[c] : 0.0;
    const double dzf = g.dzf[K - 1];
    const double du0 = (uh0 - u0) / dzf, du1 = (uh1 - u1) / dzf, dv0 = (vh0 - v0) / dzf, dv1 = (vh1 - v1) / dzf;
    const double su = 0.5 * (du0 * du0 + du1 * du1), sv = 0.5 * (dv0 * dv0 + dv1 * dv1);
    const double N2 = hy_cv_dzb(q, tl, th, sl, sh, dzf);
    const double ku = Ku[ck], kc = Kc[ck];
    if (K > 1) {
      const long cg = c - sz;                                         // centre K - 1
      const double P = (0.5 * (kul + ku)) * (0.5 * (sul + su) + 0.5 * (svl + sv));
      const double B = -(0.5 * (kcl + kc)) * (0.5 * (n2l + N2));
      G[cg] = (G[cg] + P) + B;
    }
    sul = su;
    svl = sv;
    n2l = N2;
    kul = ku;
    kcl = kc;
    u0 = uh0;
    u1 = uh1;
    v0 = vh0;
    v1 = vh1;
    tl = th;
    sl = sh;
  }
}

// HyCvCol<0> with the implicit linear term on the diagonal, the reference's order: ((1 - dt L[k]) - upper) - lower
struct HyCvColLin {
  HyCvCol<0> col;
  const double* L;          // the column's L at level 1
  long szl;

  __device__ double first(double f) {
    OCN_NO_CONTRACT
    col.up = col.g.Nz > 1 ? col.coef(2, 1, 2) : 0.0;
    col.beta = ((1.0 - col.dt * L[0]) - col.up) - 0.0;
    col.phi = f / col.beta;
    return col.phi;
  }
  __device__ double next(int K, double f) {
    OCN_NO_CONTRACT
    const double a = col.coef(K, K, K);
    const double c = col.up;
    col.up = K < col.g.Nz ? col.coef(K + 1, K, K + 1) : 0.0;
    const double b = ((1.0 - col.dt * L[(long)(K - 1) * szl]) - col.up) - a;
    const double t = c / col.beta;
    col.s.t[col.ct + (long)(K - 1) * col.st] = t;
    col.beta = b - a * t;
    col.phi = (f - a * col.phi) / col.beta;
    return col.phi;
  }
  __device__ double tk(int K) const { return col.tk(K); }
};

// k_hy_cv_implicit<0> with the linear term (the kernel-by-kernel path of the tracer e)
__global__ void k_hy_cv_implicit_lin(double* f, HyCvSolve s, HyCvLin l, HyGrid g, double dt, long sy, long sz) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= g.Nx || j >= g.Ny) return;
  HyCvColLin col{{s, g, dt, (i + g.Hx) + (long)(j + g.Hy) * s.syk + (long)g.Hz * s.szk, i + (long)j * g.Nx, (long)g.Nx * g.Ny},
                 l.L + (i + g.Hx) + (long)(j + g.Hy) * l.sy + (long)g.Hz * l.sz, l.sz};
  double* p = f + (i + g.Hx) + (long)(j + g.Hy) * sy + (long)g.Hz * sz;
  double phi = col.first(p[0]);
  p[0] = phi;
  for (int K = 2; K <= g.Nz; ++K) {
    phi = col.next(K, p[(K - 1) * sz]);
    p[(K - 1) * sz] = phi;
  }
  for (int K = g.Nz - 1; K >= 1; --K) {
    phi = p[(K - 1) * sz] - col.tk(K + 1) * phi;
    p[(K - 1) * sz] = phi;
  }
}

// k_hy_cv_ab2<0> with the linear term (the fused path of the tracer e)
__global__ void k_hy_cv_ab2_lin(double* f, const double* gn, double* gm, double dt, double cn, double cm, HyCvSolve s, HyCvLin l, HyGrid g,
                                long sy, long sz) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= g.Nx || j >= g.Ny) return;
  HyCvColLin col{{s, g, dt, (i + g.Hx) + (long)(j + g.Hy) * s.syk + (long)g.Hz * s.szk, i + (long)j * g.Nx, (long)g.Nx * g.Ny},
                 l.L + (i + g.Hx) + (long)(j + g.Hy) * l.sy + (long)g.Hz * l.sz, l.sz};
  long c = (i + g.Hx) + (long)(j + g.Hy) * sy + (long)g.Hz * sz;
  double phi = 0.0;
  for (int k = 0; k < g.Nz; ++k, c += sz) {
    const double n = gn[c];
    const double cs = hy_ab2(f[c], n, gm[c], dt, cn, cm);
    gm[c] = n;
    phi = k == 0 ? col.first(cs) : col.next(k + 1, cs);
    f[c] = phi;
  }
  c -= sz;
  for (int K = g.Nz - 1; K >= 1; --K) {
    c -= sz;
    phi = f[c] - col.tk(K + 1) * phi;
    f[c] = phi;
  }
}
