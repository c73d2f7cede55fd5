// hyconvect.h -- ConvectiveAdjustmentVerticalDiffusivity (CAVD) of the HydrostaticFreeSurfaceModel, included by splitexplicit.hip after
// HyGrid, HyBuoy and hy_ab2 (it shares their definitions and the no-contraction rule of that file's kernels).
//
//   reference (paths relative to the reference's src/)                                          here
//   TurbulenceClosures/turbulence_closure_implementations/convective_adjustment_vertical_diffusivity.jl:62-123
//                                                                                                k_hy_cv_diff (in update_state!)
//   BuoyancyModels/seawater_buoyancy.jl:171-175, buoyancy_tracer.jl:16, no_buoyancy.jl:9          hy_cv_dzb
//   TurbulenceClosures/vertically_implicit_diffusion_solver.jl:40-95, closure_tuples.jl:21-52,
//   Solvers/batched_tridiagonal_solver.jl:91-121                                                  HyCvCol; k_hy_cv_implicit,
//                                                                                                k_hy_cv_momentum, k_hy_cv_ab2
//   .../abstract_scalar_diffusivity_closure.jl:190-191, 207, 213-254, closure_kernel_operators.jl:22-47, 94-97
//                                                                                                hyclosure.h, k_hy_clo_*<.., VZ>
//
// Diffusivities.  kappa and nu are (Center, Center, Face) fields; faces 1..Nz get ifelse(d_z b >= 0, background, convective), face
// Nz + 1 and the z halos stay zero.  The reference then fills their x / y halos like any Center field (no condition in z).  Those
// fills and the band exchange copy values about, and T / S (already filled by update_state!) carry the very copies the fill of
// kappa would make, so computing kappa from T / S over the whole parent x / y range leaves the filled field -- except where no fill
// reaches (beyond the first halo cell at a wall, the corners of two walls: those stay zero), and at face 1, where the halo level 0 of
// a halo column is not filled: level 1 stands for it there, as the no-flux fill of every interior column has it.
//
// Implicit solve.  The tridiagonal coefficients of a column come from its own kappa (tracers) or nu interpolated to the velocity
// point (0.5 (nu[i-1] + nu[i]) for u, along y for v), plus the constant of a VerticalScalarDiffusivity in the same tuple (the
// tuple sums the two diagonals; two terms commute).  Every column runs the reference's modified Thomas sweep; the multipliers t_k
// wait in a scratch array (Nx Ny Nz, allocated with the closure) for the way back down.  The coefficients are non-negative, so
// beta >= 1 and the sweep's early exit cannot trigger.  Divisions are IEEE divisions, as the reference's `/`.
struct HyCvSolve {
  const double* K;     // kappa or nu, (Center, Center, Face)
  long syk, szk;
  double kv;           // VerticalScalarDiffusivity's coefficient for this field in the same tuple (0: none)
  double* t;           // scratch, Nx Ny Nz
};

// d_z b at face K between T / S values lo (level K - 1) and hi (level K), the reference's operand order
__device__ inline double hy_cv_dzb(const HyBuoy& q, double tl, double th, double sl, double sh, double dzf) {
  OCN_NO_CONTRACT
  if (q.kind == 1) return (th - tl) / dzf;
  if (q.kind == 2) return q.g * (q.alpha * ((th - tl) / dzf) - q.beta * ((sh - sl) / dzf));
  return 0.0;
}

// kappa, nu at faces 1..Nz over the parent x / y range (one thread per column, marching upwards); xb: Bounded x; ylo / yhi: this
// grid or band ends at a wall in y
__global__ void k_hy_cv_diff(HyGrid g, HyBuoy q, double kc, double nuc, double kb, double nub, const double* T, const double* S, double* kap,
                             double* nu, int Tx, int Ty, int xb, int ylo, int yhi, long sy, long sz) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= Tx || j >= Ty) return;
  // a wall's fill reaches its first halo cell only, and neither fill the corners of two walls: those cells stay zero
  const bool xh = i < g.Hx || i >= g.Hx + g.Nx, yw = (ylo && j < g.Hy) || (yhi && j >= g.Hy + g.Ny);
  const bool xfar = i < g.Hx - 1 || i > g.Hx + g.Nx, yfar = (ylo && j < g.Hy - 1) || (yhi && j > g.Hy + g.Ny);
  if ((xb && (xfar || (xh && yw))) || yfar) return;
  long c = i + (long)j * sy + (long)g.Hz * sz;
  double tl = T ? T[c] : 0.0, sl = S ? S[c] : 0.0;
  for (int k = 0; k < g.Nz; ++k, c += sz) {
    const double th = T ? T[c] : 0.0, sh = S ? S[c] : 0.0;
    const bool stable = hy_cv_dzb(q, tl, th, sl, sh, g.dzf[k]) >= 0;
    kap[c] = stable ? kb : kc;
    nu[c] = stable ? nub : nuc;
    tl = th;
    sl = sh;
  }
}

// one column of the modified Thomas sweep.  LOC: 0 a tracer (kappa as it is), 1 u (nu along x to Face), 2 v (along y); 3, 4, 5 the
// same with (Center, Center, Center) coefficients (hyribased.h), interpolated to face K from the centres K - 1 and K, after x / y
// for u / v.  ck: the coefficient field's element at face 1 (or level 1) of the column (x / y of the field point); ct: the column's
// scratch element at level 1
template <int LOC>
struct HyCvCol {
  const HyCvSolve& s;
  const HyGrid& g;
  double dt;
  long ck, ct, st;     // st: scratch stride between levels
  double beta = 0.0, phi = 0.0, up = 0.0;

  __device__ double face(int K) const {        // the coefficient at face K (1-based)
    OCN_NO_CONTRACT
    const double* p = s.K + ck + (long)(K - 1) * s.szk;
    if (LOC == 0) return p[0];
    if (LOC == 1) return 0.5 * (p[-1] + p[0]);
    if (LOC == 2) return 0.5 * (p[-s.syk] + p[0]);
    const double* m = p - s.szk;
    if (LOC == 3) return 0.5 * (m[0] + p[0]);
    if (LOC == 4) return 0.5 * (0.5 * (m[-1] + m[0]) + 0.5 * (p[-1] + p[0]));
    return 0.5 * (0.5 * (m[-s.syk] + m[0]) + 0.5 * (p[-s.syk] + p[0]));
  }
  // -dt kappa / dz^c[kc] / dz^f[kf] of this closure, plus the VerticalScalarDiffusivity's
  __device__ double coef(int K, int kc, int kf) const {
    OCN_NO_CONTRACT
    const double a = -dt * (face(K) / g.dzc[kc - 1] / g.dzf[kf - 1]);
    return s.kv != 0.0 ? -dt * (s.kv / g.dzc[kc - 1] / g.dzf[kf - 1]) + a : a;
  }
  __device__ double first(double f) {          // level 1
    OCN_NO_CONTRACT
    up = g.Nz > 1 ? coef(2, 1, 2) : 0.0;       // ivd_upper_diagonal(1): face 2
    beta = (1.0 - up) - 0.0;                   // ivd_diagonal(1), ivd_lower_diagonal(0) = 0
    phi = f / beta;
    return phi;
  }
  __device__ double next(int K, double f) {    // level K = 2..Nz
    OCN_NO_CONTRACT
    const double a = coef(K, K, K);            // ivd_lower_diagonal(K - 1): face K
    const double c = up;                       // ivd_upper_diagonal(K - 1)
    up = K < g.Nz ? coef(K + 1, K, K + 1) : 0.0;
    const double b = (1.0 - up) - a;
    const double t = c / beta;
    s.t[ct + (long)(K - 1) * st] = t;
    beta = b - a * t;
    phi = (f - a * phi) / beta;
    return phi;
  }
  __device__ double tk(int K) const { return s.t[ct + (long)(K - 1) * st]; }
};

// implicit_step! of one field (the kernel-by-kernel path): over the grid's cells, one thread per column
template <int LOC>
__global__ void k_hy_cv_implicit(double* f, HyCvSolve s, HyGrid g, double dt, long sy, long sz) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= g.Nx || j >= g.Ny) return;
  HyCvCol<LOC> col{s, g, dt, (i + g.Hx) + (long)(j + g.Hy) * s.syk + (long)g.Hz * s.szk, i + (long)j * g.Nx, (long)g.Nx * g.Ny};
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

// k_hy_momentum with this closure's solve: the barotropic mode of the velocity before the step (-> U), the vertical integral of the
// AB2 tendency (-> G^U), the AB2 step feeding the forward elimination, G^- <- G^n; then the back substitution and the barotropic
// mode of the stepped, solved column (-> Un).  Sums over the field's interior, the step over the grid's cells
template <int LOC>
__global__ void k_hy_cv_momentum(double* u, const double* gn, double* gm, double* U, double* GU, double* Un, double dt, double cn, double cm,
                                 HyCvSolve s, HyGrid g, int Sx, int Sy, long sy3, long sz3, long sy2) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= Sx || j >= Sy) return;
  const bool step = i < g.Nx && j < g.Ny;
  const long c0 = (i + g.Hx) + (long)(j + g.Hy) * sy3 + (long)g.Hz * sz3;
  HyCvCol<LOC> col{s, g, dt, (i + g.Hx) + (long)(j + g.Hy) * s.syk + (long)g.Hz * s.szk, i + (long)j * g.Nx, (long)g.Nx * g.Ny};
  long c = c0;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, phi = 0.0;
  for (int k = 0; k < g.Nz; ++k, c += sz3) {
    const double uo = u[c], n = gn[c], m = gm[c], dz = g.dzc[k];
    const double G = cn * n - cm * m;
    const double un = step ? hy_ab2(uo, n, m, dt, cn, cm) : uo;
    a0 = k == 0 ? uo * dz : a0 + uo * dz;
    a1 = k == 0 ? G * dz : a1 + G * dz;
    a2 = k == 0 ? un * dz : a2 + un * dz;
    if (step) {
      phi = k == 0 ? col.first(un) : col.next(k + 1, un);
      u[c] = phi;
      gm[c] = n;
    }
  }
  if (step) {
    c = c0 + (long)(g.Nz - 1) * sz3;
    for (int K = g.Nz - 1; K >= 1; --K) {
      c -= sz3;
      phi = u[c] - col.tk(K + 1) * phi;
      u[c] = phi;
    }
    c = c0;
    for (int k = 0; k < g.Nz; ++k, c += sz3) {
      const double q = u[c] * g.dzc[k];
      a2 = k == 0 ? q : a2 + q;
    }
  }
  const long c2 = (i + g.Hx) + (long)(j + g.Hy) * sy2;
  U[c2] = a0;
  GU[c2] = a1;
  Un[c2] = a2;
}

// a tracer: AB2 step, G^- <- G^n and this closure's solve in one kernel (LOC 0, or 3 for (Center, Center, Center) coefficients)
template <int LOC = 0>
__global__ void k_hy_cv_ab2(double* f, const double* gn, double* gm, double dt, double cn, double cm, HyCvSolve s, HyGrid g, long sy, long sz) {
  OCN_NO_CONTRACT
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= g.Nx || j >= g.Ny) return;
  HyCvCol<LOC> col{s, g, dt, (i + g.Hx) + (long)(j + g.Hy) * s.syk + (long)g.Hz * s.szk, i + (long)j * g.Nx, (long)g.Nx * g.Ny};
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
