// hyfftfs.h -- ImplicitFreeSurface(solver_method = :FastFourierTransform) of the hydrostatic model on a horizontally regular
// rectilinear grid (included by splitexplicit.hip after hyimplicit.h).
//
//   reference (paths relative to its src/)                                                      here
//   Models/HydrostaticFreeSurfaceModels/fft_based_implicit_free_surface_solver.jl:111-116 (rhs)  k_ffs_x_fwd
//   .../fft_based_implicit_free_surface_solver.jl:80-92 (m = -1 / (g Lz Δt²))                    ffs_solve
//   Solvers/fft_based_poisson_solver.jl:93-120 (forward, ϕ̂ = -b̂ / (λx + λy - m), inverse)       k_ffs_x_fwd, k_ffs_y_solve, k_ffs_x_inv
//   Solvers/poisson_eigenvalues.jl, plan_transforms.jl (DFT for Periodic, REDFT10 / REDFT01)     ocn_ifs_create_fft (tables), ffs_line
//   fill_halo_regions!(η)                                                                        k_ffs_fill
//
// The solve is direct:  (∇² + m) η = rhs  with the eigenfunctions of the discrete ∇² in x and y.  The plane is a few MB at most, so
// the cost is the chain of dependent launches, as for the PCG it replaces; there are four, and nothing is read back:
//   k_ffs_x_fwd    a row per line: forms rhs from ∫ᶻQ and η while loading (and stores it), transforms the row along x in LDS;
//   k_ffs_y_solve  a group of adjacent x-coefficients per workgroup (loads coalesced along x): forward y transform, the division by
//                  λx + λy - m, inverse y transform, in place;
//   k_ffs_x_inv    inverse x transform per row, η's interior;
//   k_ffs_fill     η's halos in one launch: every halo cell copies the cell the library's two fills would copy (ifs_src).
//
// Everything between the transforms is REAL.  The data are real and so are the eigenvalues, so the x-spectrum of a row is kept as
// Nx real numbers: the DCT-II coefficients for Bounded x, and for Periodic x the half-complex form S[p] = Re Z[p] (p <= N/2),
// S[p] = Im Z[N - p] (p > N/2), whose eigenvalue λ[p] = λ[N - p] is the one of either part.  The y transform of such a column is the
// transform of a real column.  A line is transformed as a complex line with a zero imaginary part (a line of complex doubles and
// its ping-pong buffer: 32 N bytes of LDS, 128 KB at the longest line of 4096):
//   Periodic  Z = DFT(x); back x = Re IDFT(Z) / N;
//   Bounded   the DCT-II through one DFT of the same length (Makhoul 1980): v[n] = x[2n], v[N-1-n] = x[2n+1], V = DFT(v),
//             X[k] = 2 Re(e^{-iπk/2N} V[k]) = REDFT10(x)[k];  back V[k] = e^{iπk/2N} (X[k] - i X[N-k]) / 2 (X[N] = 0), v = IDFT(V) / N.
// The DFT is a Stockham autosort transform of radices 4, 2, 3, 5 for N = 2^a 3^b 5^c ("fast"), and the plain O(N²) sum over the same
// table of roots for every other N ("direct").  Roots, phases and eigenvalues come from tables built on the host in double precision;
// no sine or cosine is evaluated on the device.  The 1 / (Nx Ny) of the two inverse transforms is folded into the division.
//
// This solve is compared to rounding, not bit for bit (the reference runs FFTW), so contraction into FMAs is left to the compiler.
// It is deterministic: no atomics, and every sum has one fixed order.
#pragma once

#define FFS_NT 256          // threads per workgroup
#define FFS_NMAX 4096       // longest line: 2 x 4096 complex doubles = 128 KB of the CU's 160 KB LDS
#define FFS_MAXST 12        // stages at most (4096 = 4^6; 3^7 = 2187 and 2 x 3^7 > 4096; a radix-2 stage at most once)

struct ffs_c {
  double x, y;
};

struct FfsDir {
  int N, bounded, fast, nst;
  int rad[FFS_MAXST];
  const ffs_c* tw;       // e^{-2πi q / N}, q = 0..N-1
  const ffs_c* ph;       // e^{-iπ k / 2N}, k = 0..N-1 (Bounded)
  const double* lam;     // the eigenvalue of the stored coefficient p = 0..N-1
};

__device__ inline ffs_c ffs_mul(ffs_c a, ffs_c b) { return ffs_c{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
// position of sample i in the line a Bounded direction transforms (Makhoul's even-odd permutation); Periodic: i
__device__ inline int ffs_pos(const FfsDir& d, int i) { return d.bounded ? ((i & 1) ? d.N - 1 - (i >> 1) : (i >> 1)) : i; }

// one Stockham stage of radix R on a line: M = N / R butterflies shared by the TL threads of the line; sg = +1 forward, -1 inverse
template <int R>
__device__ inline void ffs_stage(const ffs_c* in, ffs_c* out, const FfsDir& d, int Ns, double sg, int tl, int TL) {
  const int N = d.N, M = N / R, tws = N / (Ns * R);
  ffs_c w[R];                                   // the R-th roots of unity
  for (int q = 0; q < R; ++q) {
    w[q] = d.tw[q * M];
    w[q].y *= sg;
  }
  for (int j = tl; j < M; j += TL) {
    const int k = j % Ns;
    ffs_c a[R];
    for (int t = 0; t < R; ++t) {
      ffs_c v = in[j + t * M];
      if (t && k) {
        ffs_c c = d.tw[(t * k * tws) % N];
        c.y *= sg;
        v = ffs_mul(v, c);
      }
      a[t] = v;
    }
    const int j0 = (j - k) * R + k;
    for (int t = 0; t < R; ++t) {
      ffs_c s = a[0];
      for (int q = 1; q < R; ++q) {
        const ffs_c p = ffs_mul(a[q], w[(q * t) % R]);
        s.x += p.x;
        s.y += p.y;
      }
      out[j0 + t * Ns] = s;
    }
  }
}

// the DFT of the block's lines, every thread of the block calls it (the barriers are the block's): line in a, scratch b; on return
// a points at the result.  act: this thread's line exists.
__device__ inline void ffs_line(ffs_c*& a, ffs_c*& b, const FfsDir& d, double sg, int tl, int TL, bool act) {
  if (d.fast) {
    int Ns = 1;
    for (int s = 0; s < d.nst; ++s) {
      const int R = d.rad[s];
      if (act) {
        if (R == 4) ffs_stage<4>(a, b, d, Ns, sg, tl, TL);
        else if (R == 2) ffs_stage<2>(a, b, d, Ns, sg, tl, TL);
        else if (R == 3) ffs_stage<3>(a, b, d, Ns, sg, tl, TL);
        else ffs_stage<5>(a, b, d, Ns, sg, tl, TL);
      }
      Ns *= R;
      __syncthreads();
      ffs_c* t = a; a = b; b = t;
    }
  } else {
    const int N = d.N;
    if (act)
      for (int k = tl; k < N; k += TL) {
        ffs_c s{0.0, 0.0};
        int q = 0;                              // (k n) mod N
        for (int n = 0; n < N; ++n) {
          ffs_c c = d.tw[q];
          c.y *= sg;
          const ffs_c p = ffs_mul(a[n], c);
          s.x += p.x;
          s.y += p.y;
          q += k;
          if (q >= N) q -= N;
        }
        b[k] = s;
      }
    __syncthreads();
    ffs_c* t = a; a = b; b = t;
  }
}

// the stored real coefficient p of a transformed line (half-complex for Periodic, REDFT10 for Bounded)
__device__ inline double ffs_coef(const ffs_c* Z, const FfsDir& d, int p) {
  if (d.bounded) {
    const ffs_c w = d.ph[p], v = Z[p];
    return 2.0 * (w.x * v.x - w.y * v.y);
  }
  return 2 * p <= d.N ? Z[p].x : Z[d.N - p].y;
}
// the complex line to transform back, entry k, from the stored coefficients S (stride st)
__device__ inline ffs_c ffs_uncoef(const double* S, long st, const FfsDir& d, int k) {
  const int N = d.N;
  if (d.bounded) {
    const double xr = S[k * st], xi = k ? S[(N - k) * st] : 0.0;
    const ffs_c w = d.ph[k];                    // conj(w) (xr - i xi) / 2
    return ffs_c{0.5 * (w.x * xr - w.y * xi), 0.5 * (-w.x * xi - w.y * xr)};
  }
  const int q = k < N - k ? k : N - k;
  const double re = S[q * st];
  double im = (q == 0 || 2 * q == N) ? 0.0 : S[(N - q) * st];
  if (k != q) im = -im;
  return ffs_c{re, im};
}

struct FfsGeo {
  int Nx, Ny, Hx, Hy, Tx;      // η's parent row length Tx
  long su, sv;                 // row strides of ∫ᶻQ.u and ∫ᶻQ.v
};

// ---- rhs and the forward x transform: L rows per workgroup, FFS_NT / L threads per row ------------------------------------------
// rhs = (δx ∫ᶻQ.u + δy ∫ᶻQ.v - Az η / Δt) / (g Lz Δt Az); spec: Ny rows of Nx coefficients, no halos
template <int CAP>
__global__ void __launch_bounds__(FFS_NT) k_ffs_x_fwd(FfsGeo g, FfsDir d, int L, const double* eta, const double* Qu, const double* Qv,
                                                      const double* azcc, double* rhs, double* spec, double dt, double glzdt) {
  OCN_SHARED ffs_c lds[2 * CAP];
  const int TL = FFS_NT / L, l = threadIdx.x / TL, tl = threadIdx.x % TL, j = blockIdx.x * L + l, N = d.N;
  const bool act = j < g.Ny;
  ffs_c *a = lds + l * N, *b = lds + CAP + l * N;
  if (act) {
    const int r = j + g.Hy;
    const double az = azcc[r];
    for (int i = tl; i < N; i += TL) {
      const int c = i + g.Hx;
      const long P = c + (long)r * g.Tx;
      const double dQ = (Qu[(c + 1) + r * g.su] - Qu[c + r * g.su]) + (Qv[c + (r + 1) * g.sv] - Qv[c + r * g.sv]);
      const double v = (dQ - az * eta[P] / dt) / (glzdt * az);
      rhs[P] = v;
      a[ffs_pos(d, i)] = ffs_c{v, 0.0};
    }
  }
  __syncthreads();
  ffs_line(a, b, d, 1.0, tl, TL, act);
  if (act)
    for (int p = tl; p < N; p += TL) spec[p + (long)j * N] = ffs_coef(a, d, p);
}

// ---- forward y transform, division, inverse y transform: L adjacent x-coefficients per workgroup ----------------------------------
// global loads and stores run with the coefficient index fastest (c = thread % L), the transforms with FFS_NT / L threads per column
template <int CAP>
__global__ void __launch_bounds__(FFS_NT) k_ffs_y_solve(FfsDir d, int L, int Nx, const double* lamx, double* spec, double m, double norm) {
  OCN_SHARED ffs_c lds[2 * CAP];
  const int TL = FFS_NT / L, l = threadIdx.x / TL, tl = threadIdx.x % TL, N = d.N;
  const int c = threadIdx.x % L, n0 = threadIdx.x / L, nstep = FFS_NT / L, p0 = blockIdx.x * L;
  const bool act = p0 + l < Nx;
  if (p0 + c < Nx)
    for (int n = n0; n < N; n += nstep) lds[c * N + ffs_pos(d, n)] = ffs_c{spec[(p0 + c) + (long)n * Nx], 0.0};
  __syncthreads();
  ffs_c *a = lds + l * N, *b = lds + CAP + l * N;
  ffs_line(a, b, d, 1.0, tl, TL, act);
  const double lx = act ? lamx[p0 + l] : 0.0;
  if (d.bounded) {
    // the scaled DCT coefficients as reals in the scratch line, then the line to transform back
    double* X = (double*)b;
    if (act)
      for (int k = tl; k < N; k += TL) X[k] = ffs_coef(a, d, k) * (-norm / ((lx + d.lam[k]) - m));
    __syncthreads();
    if (act)
      for (int k = tl; k < N; k += TL) a[k] = ffs_uncoef(X, 1, d, k);
    __syncthreads();
  } else {
    if (act)
      for (int k = tl; k < N; k += TL) {
        const double s = -norm / ((lx + d.lam[k]) - m);
        a[k].x *= s;
        a[k].y *= s;
      }
    __syncthreads();
  }
  ffs_line(a, b, d, -1.0, tl, TL, act);
  // every line of the block ends in the same buffer
  const ffs_c* res = a - l * N;
  if (p0 + c < Nx)
    for (int n = n0; n < N; n += nstep) spec[(p0 + c) + (long)n * Nx] = res[c * N + ffs_pos(d, n)].x;
}

// ---- inverse x transform, η's interior ----------------------------------------------------------------------------------------------
template <int CAP>
__global__ void __launch_bounds__(FFS_NT) k_ffs_x_inv(FfsGeo g, FfsDir d, int L, const double* spec, double* eta) {
  OCN_SHARED ffs_c lds[2 * CAP];
  const int TL = FFS_NT / L, l = threadIdx.x / TL, tl = threadIdx.x % TL, j = blockIdx.x * L + l, N = d.N;
  const bool act = j < g.Ny;
  ffs_c *a = lds + l * N, *b = lds + CAP + l * N;
  if (act)
    for (int k = tl; k < N; k += TL) a[k] = ffs_uncoef(spec + (long)j * N, 1, d, k);
  __syncthreads();
  ffs_line(a, b, d, -1.0, tl, TL, act);
  if (act)
    for (int i = tl; i < N; i += TL) eta[(i + g.Hx) + (long)(j + g.Hy) * g.Tx] = a[ffs_pos(d, i)].x;
}

// ---- fill_halo_regions!(η) in one launch: a halo cell takes the interior cell the library's fills would copy into it -------------
__global__ void k_ffs_fill(IfsGeo g, double* eta) {
  const int P = blockIdx.x * blockDim.x + threadIdx.x;
  if (P >= g.Tx * g.Ty) return;
  const int j = P / g.Tx, i = P - j * g.Tx;
  if (i >= g.Hx && i < g.Hx + g.Nx && j >= g.Hy && j < g.Hy + g.Ny) return;
  const long s = ifs_src(g, i, j);
  if (s != P) eta[P] = eta[s];
}
