// internal.h -- host-side objects behind the opaque handles of include/ocnhip.h
#pragma once
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/ocnhip.h"
#include "compat.h"
#include "stencils.h"

#define OCN_NF (3 + OCN_MAX_TRACERS)
// ocn_model::d.closure of a model made by ocn_model_create_smagorinsky_lilly (never in a caller's ocn_model_desc): the eddy
// viscosity field nu_e of SmagorinskyLilly; d.nu / d.kappa hold the molecular part of the (SmagorinskyLilly,
// ScalarDiffusivity) tuple, or zero
#define OCN_CLOSURE_SMAG 3

struct ProfPhase {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  double total_ms = 0;
  int64_t count = 0;
};

struct ocn_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  char err[512] = {0};
  bool profiling = false;
  std::map<std::string, ProfPhase> prof;
  std::string prof_only;   // when set, only this phase records events (each record costs ~4 us of stream time)
  // multi-GPU
  int rank = 0, nranks = 1;
  void* comm = nullptr;  // ncclComm_t
  void* shm = nullptr;   // ShmWorld: host shared-memory transport (tests / rehearsals on one GPU or none), comm.hip
  // z-slab halo exchange overlapped with the interior levels of the next tendency kernel (api.hip fused_substep): the
  // exchange runs on its own stream between two events
  bool overlap_ready = false;
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_main = nullptr, ev_halo = nullptr, ev_halo2 = nullptr;
  std::vector<struct ocn_model*> models;   // live models (ocn_sync settles their exchanges)
  int sticky_rc = 0;   // first failure of an exchange issued from a helper that cannot return it (splitexplicit.hip hfield_fill); reported by the entry point
};

void ocn_set_error(ocn_ctx* ctx, const char* fmt, ...);

struct CommOp {
  void* buf;
  size_t bytes;
  int peer;
  int tag;
};

struct ocn_grid {
  ocn_ctx* ctx;
  int Nzg = 0;          // global Nz (N[2] is this rank's slab)
  bool dist = false;    // z-slab decomposition active (also forced with one rank by OCNHIP_FORCE_DIST=1)
  int Nyg = 0;          // global Ny (N[1] is this rank's slab when dist_y)
  bool dist_y = false;  // y-slab decomposition (Bounded z: every rank keeps whole columns)
  ocn_grid_desc d;
  int N[3], H[3], topo[3];
  int PH[3];            // physical halo: H, except Flat x / y, which are stored with broadcast halos
  double L[3], x0[3];
  bool z_regular;
  std::vector<double> zF_int;            // interior faces (stretched)
  std::vector<double> h_dzc, h_dzf;      // host spacings incl. halos (stretched), layout as GridDev
  double* d_dzc = nullptr;
  double* d_dzf = nullptr;
  double *d_rdzc = nullptr, *d_rdzf = nullptr;
  GridDev dev;                           // for the current halo
};

struct BCdev {
  int kind;
  double value;
  const double* arr;  // device (Nx*Ny) or null
};

// Device layout of a field.  T is the reference's parent size (Grids/new_data.jl:16-61); P the size actually
// allocated.  They coincide unless x or y is Bounded or Flat: then every field of the model shares ONE pitch
// (as hipMallocPitch would give) -- Nx+2H+1 columns when x is Bounded, so Face- and Center-located fields have
// equal strides and one linear index addresses all of them -- and a Flat x / y direction is stored with
// broadcast halos (every difference across it is exactly 0, every interpolation the identity, as the
// reference's Flat operators).  ocn_field_layout() reports strides and origin; upload / download convert.
struct Field {
  double* d = nullptr;  // parent array on the device
  int T[3] = {0, 0, 0};
  int P[3] = {0, 0, 0};
  int off[3] = {0, 0, 0};   // physical index of the logical parent's first element
  int loc[3] = {0, 0, 0};
  size_t n = 0;             // physical element count
  BCdev bc[6];
  bool present = false;
  double* interior() const;  // pointer to the first interior cell
  long sy = 0, sz = 0;
  int Hx = 0, Hy = 0, Hz = 0;
};

struct PoissonSolver;

// Column tables of one feature: [3 stage slots][nitem][len] doubles on the device, library-owned host staging of the same shape
// and one event per (slot, item), recorded behind that item's upload.  A setter copies the caller's runs into the staging memory
// (the caller's arrays are free again on return) and queues one asynchronous copy on the context's stream; the next upload of
// the same (slot, item) waits for that copy alone -- it was queued ahead of the step that used it, so this never waits for the
// stream to drain.  The device addresses never change, so a captured step graph keeps reading the current contents.  (api.hip)
struct StagedTables {
  int nitem = 0;
  size_t len = 0;
  double *dev = nullptr, *stage = nullptr;
  hipEvent_t ev[3][OCN_NF] = {};
  bool alloc(int items, size_t length);   // zero-filled; false: out of memory
  double* slot(int s, int item) const { return dev + ((size_t)s * nitem + item) * len; }
  // nruns runs of runlen doubles, back to back from the start of the item; a null run is a run of zeros
  int upload(ocn_ctx* ctx, int s, int item, const double* const* runs, int nruns, size_t runlen);
  void release();
};

struct ocn_model {
  ocn_grid* g;
  ocn_ctx* ctx;
  ocn_model_desc d;
  GridDev gd;
  int nt;  // tracers
  Field u, v, w, pHY, pNHS;
  Field tr[OCN_MAX_TRACERS], Gn[OCN_NF], Gm[OCN_NF];
  Field nu_e, kappa_e[OCN_MAX_TRACERS];
  // projection scratch: predictor velocities are written here by the fused kernels
  Field us, vs, ws;
  Field trs[OCN_MAX_TRACERS];   // second tracer buffers of the fused path
  PoissonSolver* solver = nullptr;
  std::vector<double*> owned;  // extra device allocations (bc arrays)
  // clock / stepper state
  double time = 0, previous_dt = INFINITY;
  int64_t iteration = 0;
  int stage = 1;
  double* d_red = nullptr;  // reduction scratch
  int fast_path = 0;        // 1: fused periodic WENO kernels usable
  int bz_fast = 0;          // 1: Bounded z: tiled advection + update kernel on top of the general kernels' other terms
  double* amd_tab = nullptr;     // per-level factors of the AMD predictors (kernels.hip amd_build_table)
  // SmagorinskyLilly (smagorinsky.hip): C, Cb, 1 / Pr per tracer (kappa_e = nu_e / Pr is never stored) and the per-level table
  double smag_C = 0, smag_Cb = 0, smag_rPr[OCN_MAX_TRACERS] = {0};
  double* smag_tab = nullptr;    // [Nz]: (C Delta_f)^2 of interior level k, entry [k] (smag_build_table)
  int knob_no_smag_tiled = 0;    // OCNHIP_NO_SMAG_TILED=1: the one-thread-per-cell nu_e kernel everywhere (tests, A/B)
  double* phi_below = nullptr;   // (Nx,Ny): top plane of the lower neighbour's pressure (slab runs)
  double *ypack_s = nullptr, *ypack_r = nullptr;   // y-slab halo exchange staging (send / receive)
  size_t ypack_n = 0;
  bool gn_alias_gm = false; // after a fused AB2 step G^n and G^- are the same buffer (pointer swap instead of a copy)
  // Bounded-z tiled path: between the time-stepper update and the projection the predictor U* lives in us / vs / ws;
  // the projection writes u = U* - dt grad p back into u, v, w, so their device pointers never change.
  bool pred_active = false;
  ocn_grid* own_grid = nullptr;   // private copy of the caller's grid when the advection scheme needs wider halos
  int knob_fused_xt = 0, knob_no_dma = 0, knob_no_tracer3 = 0, knob_prio = 0x20FF;   // fused_read_knobs(), at creation
  // whole-step hipGraphs of the general path (api.hip step_graphed): one entry per distinct (dt, stepper state, buffer rotation)
  // whole-step hipGraph cache: `key` is a hash of `words` (dt bits, stepper flags, the device pointer of every rotating buffer);
  // a hit on the hash is only taken after the words themselves compare equal
  struct StepGraph { uint64_t key; int seen; void* exec; std::vector<uint64_t> words; };
  std::vector<StepGraph> graphs;
  int knob_overlap_cus = 16; // CUs the interior tendency launch leaves to the communication kernels (OCNHIP_OVERLAP_CUS)
  int knob_overlap = -1;     // OCNHIP_OVERLAP=0|1: z-slab halo exchange overlapped with the next tendency launch (default: with > 1 rank)
  bool halo_inflight = false, halo2_inflight = false;   // exchange of (u, v, w, tracers) started, not yet waited for (halo2: unused since round 3)
  // z-slab runs of the all-in-one path: nothing inside a time step reads the z halos of pNHS (the projection takes the one plane
  // it needs through fused_exchange_phi), so their exchange -- 2 x H planes per step -- is deferred until somebody can look:
  // ocn_sync, ocn_fill_halos(pNHS) and ocn_field_download(pNHS), all collective on slab runs (api.hip pnhs_refresh)
  bool pnhs_halo_stale = false;
  int knob_split_y = 1;      // OCNHIP_SPLIT_Y=0: the periodic solve keeps its two y passes where the split-y form would serve (tests, A/B)
  int knob_xfft_team = 0;    // OCNHIP_XFFT_TEAM=1: the fused rhs + x transform loads in team order (the older variant; tests)
  int knob_graph = 1;        // OCNHIP_NO_GRAPH=1 clears it (model creation)
  int knob_tend4_vsel = 0;   // OCNHIP_TEND4_VSEL=1: k_tend4 selects stencil values, not addresses, everywhere (tests, A/B)
  int knob_locality = 1;     // OCNHIP_LOCALITY=0: k_tend4's once-touched streams (G^- loads, G^n / U* stores) keep the default cache policy
  // Single-rank all-in-one path: nothing inside a time step reads pNHS (the projection takes its gradient from the solver's real
  // buffer, the next solve overwrites it), so the projection leaves its store out and the field is written when somebody can
  // look (api.hip pnhs_materialize).  pnhs_deferred set => the solver's real buffer holds exactly the values an eager
  // projection would have stored in pNHS, and pNHS itself is out of date.  Whoever overwrites that buffer outside
  // fused_substep materialises first (or clears the flag where it writes a complete new pNHS itself).
  bool pnhs_deferred = false;
  bool pnhs_escaped = false;     // ocn_field_device_ptr(pNHS) was called: reads can no longer be seen, every projection stores
  int knob_eager_pressure = 0;   // OCNHIP_EAGER_PRESSURE=1: every projection stores pNHS (callers who read it after every step)
  // The features' functions of (z, t) arrive as host tables, one set per stage slot (StagedTables above).  UniformStokesDrift
  // (ocn_model_set_stokes_drift): six runs of Nz doubles: d_z u^s, d_z v^s at centres, at faces k = 1..Nz, d_t u^s, d_t v^s at centres.
  int stokes = 0;                // created with Stokes drift (decides the path: never the all-in-one periodic one)
  StagedTables stokes_tab;       // [3][1][6 Nz]
  // Forcing (ocn_model_create_forced): G_phi += sigma (tau - phi) + F for the fields of the two masks (bit f: u, v, w, tracers).
  // Column form: per declared field (force_ci[f]: its rank among them) sigma, tau, F as three runs of Nz doubles.  Field form: up
  // to three arrays per field in the layout of its parent array (the tiled kernels read them at the cell's own byte offset, the
  // general kernels at its interior index); an absent one is null and its load skipped.  They are part of the step graphs' key.
  uint32_t force_col = 0, force_fld = 0;
  int force_ci[OCN_NF];
  StagedTables force_tab;                // [3][declared fields][3 Nz]
  double* force_arr[OCN_NF][3] = {};     // field form: sigma, tau, F
  // BackgroundFields (ocn_model_create_background): G_phi -= div(adv, (U, V, W), phi) + div(adv, (u, v, w), Phi) with background
  // velocities U, V, W (members 0, 1, 2) and background tracers (member 3 + t).  A member has one form.  Column form: per declared
  // member (bg_ci[f]: its rank among them) one table as long as the tallest parent array; the first T[2] of the member's field are
  // used, halo levels included.  Field form: one array in that field's parent layout, allocated at creation (zero until set).
  uint32_t bg_col = 0, bg_fld = 0;
  int bg_ci[OCN_NF];
  StagedTables bg_tab;             // [3][declared members][max T[2]]
  double* bg_arr[OCN_NF] = {};     // field form
  // Tilted gravity, ConstantCartesianCoriolis, quadratic drag (ocn_model_create_tilted): the descriptor as given.  tilt_terms: a
  // gravity vector or a Cartesian rotation is set, so the TILT instantiations of k_tend_uvw / k_rest4 (and, with a gravity vector,
  // of k_hydrostatic*) serve the model; drag_any: k_drag_flux launches behind the flux-boundary kernels.
  ocn_tilted_desc tl = {};
  bool tilt_terms = false, drag_any = false;
  bool graph_off = false;    // a capture failed: this model steps launch by launch from then on
  int64_t graph_replays = 0;
};
extern thread_local int g_ocn_capturing, g_ocn_capture_poison;   // a library call that cannot be captured sets the poison flag
inline Field& pred_u(ocn_model* m) { return m->pred_active ? m->us : m->u; }
inline Field& pred_v(ocn_model* m) { return m->pred_active ? m->vs : m->v; }
inline Field& pred_w(ocn_model* m) { return m->pred_active ? m->ws : m->w; }
// the model's projections leave the pNHS store to pnhs_materialize (see pnhs_deferred)
inline bool pnhs_lazy(const ocn_model* m) { return m->fast_path && !m->g->dist && !m->knob_eager_pressure && !m->pnhs_escaped; }

// the Stokes-drift tables a tendency launch reads: the slot of the current stage (null: no Stokes drift)
inline const double* stokes_slot(const ocn_model* m) { return m->stokes ? m->stokes_tab.slot(m->stage - 1, 0) : nullptr; }
// the column tables of u, v, w of the current stage, nine runs of Nz doubles (k_rest4): when one of the three is declared all three
// have tables -- they are the first three of a slot -- and an undeclared one's stay zero.  Null: none of them is declared.
inline const double* force_col3(const ocn_model* m) { return (m->force_col & 7u) ? m->force_tab.slot(m->stage - 1, 0) : nullptr; }
inline bool model_forced(const ocn_model* m) { return (m->force_col | m->force_fld) != 0; }
// what a tendency launch reads for field f (0, 1, 2: u, v, w; 3 + t: tracer t): the column tables of the current stage and the
// field-form arrays, as parent bases (tiled kernels) or moved to the first interior cell (general kernels)
inline ForceDev force_of(const ocn_model* m, int f, bool interior) {
  ForceDev fo = {nullptr, nullptr, nullptr, nullptr};
  if (m->force_col >> f & 1u) fo.col = m->force_tab.slot(m->stage - 1, m->force_ci[f]);
  if (m->force_fld >> f & 1u) {
    const Field& F = f == 0 ? m->u : f == 1 ? m->v : f == 2 ? m->w : m->tr[f - 3];
    const size_t org = interior ? (size_t)(F.interior() - F.d) : 0;
    fo.fs = m->force_arr[f][0] ? m->force_arr[f][0] + org : nullptr;
    fo.ft = m->force_arr[f][1] ? m->force_arr[f][1] + org : nullptr;
    fo.ff = m->force_arr[f][2] ? m->force_arr[f][2] + org : nullptr;
  }
  return fo;
}

// What the TILT instantiations read, the trailing argument of k_tend_uvw / k_rest4 / k_hydrostatic* (the plain instantiations never
// look at it): the gravity unit vector and the buoyancy model's tracers (tilt), the rotation vector (cart).  Wave-uniform.
struct TiltDev {
  double gx, gy, gz, fx, fy, fz;
  int tilt, cart, buoyancy;
  double g, alpha, beta;
  const double *b, *T, *S;   // interior pointers (general kernels) or parent bases (k_rest4)
};
inline TiltDev tilt_of(const ocn_model* m, bool interior) {
  TiltDev t;
  memset(&t, 0, sizeof(t));
  if (!m->tilt_terms) return t;
  t.tilt = m->tl.has_gravity_vector;
  t.cart = m->tl.coriolis_cartesian;
  t.gx = m->tl.gx; t.gy = m->tl.gy; t.gz = m->tl.gz;
  t.fx = m->tl.fx; t.fy = m->tl.fy; t.fz = m->tl.fz;
  t.buoyancy = m->d.buoyancy;
  t.g = m->d.g; t.alpha = m->d.alpha; t.beta = m->d.beta;
  auto base = [&](int idx) -> const double* { return idx < 0 ? nullptr : interior ? m->tr[idx].interior() : m->tr[idx].d; };
  if (t.tilt) { t.b = base(m->d.b_index); t.T = base(m->d.T_index); t.S = base(m->d.S_index); }
  return t;
}

inline bool model_background(const ocn_model* m) { return (m->bg_col | m->bg_fld) != 0; }
// the field whose nodes and parent layout background member f has (0, 1, 2: u, v, w; 3 + t: tracer t)
inline const Field& bg_field_of(const ocn_model* m, int f) { return f == 0 ? m->u : f == 1 ? m->v : f == 2 ? m->w : m->tr[f - 3]; }

Field* model_field(ocn_model* m, int id);

// ---- background.hip ---------------------------------------------------------------------------------
void launch_background(ocn_model* m);   // adds the background-field advection terms to G^n of u, v, w and the tracers

// ---- kernels.hip ------------------------------------------------------------------------------------
struct FieldPtrs {   // up to velocities + both pressures + all tracers in one call (ocn_fill_halos)
  double* p[OCN_NF + 2];
  int Tx[OCN_NF + 2], Ty[OCN_NF + 2], Tz[OCN_NF + 2];   // extents the fill sweeps (the field's own parent extents)
  int n;
};
void launch_fill_periodic(ocn_model* m, const FieldPtrs& f, int dim);
void launch_fill_flat(ocn_model* m, const FieldPtrs& f, int dim);
bool launch_fill_periodic_xy(ocn_model* m, const FieldPtrs& f);   // false: not applicable, use the two passes
void launch_fill_bounded(ocn_model* m, Field** fs, int n, int dim);
void launch_tendencies(ocn_model* m, bool skip_momentum_advection = false, bool skip_tracer_advection = false);
void launch_step(ocn_model* m, double dt, double cn, double cm, int use_m, bool tracers_only = false);
void launch_store(ocn_model* m);
void launch_rhs(ocn_model* m, double dt, double* rhs, int mult_dz);
void launch_pcorrect(ocn_model* m, double dt);
void launch_hydrostatic(ocn_model* m);
void launch_copy_to_field(ocn_model* m, const double* src, Field& f);
void launch_maxdiv(ocn_model* m, double* out_dev);
void launch_amd(ocn_model* m);
int amd_build_table(ocn_model* m);

// ---- smagorinsky.hip --------------------------------------------------------------------------------
int smag_build_table(ocn_model* m);
void launch_smag(ocn_model* m);            // nu_e of SmagorinskyLilly (interior); the caller fills its halos
bool smag_tiled_ok(const ocn_model* m);    // k_smag_nu applies (else the one-thread-per-cell kernel)

// ---- fused.hip -----------------------------------------------------------------------------------------
void fused_read_knobs(ocn_model* m);
void fused_describe(const ocn_model* m, char* buf, size_t n);
bool fused_available(const ocn_model* m);
bool fused_bz_available(const ocn_model* m);
void launch_fused_bz(ocn_model* m, double dt, double cn, double cm, int use_m);
bool launch_rest4(ocn_model* m);
bool rest4_ok(const ocn_model* m);         // k_rest4 serves the model's non-advective momentum terms
int fused_cu_count(const ocn_model* m);    // compute units of the model's device (one workgroup of a marching kernel per CU)
bool fused_tracer3_ok(const ocn_model* m);
bool tracer_rest_shell(const ocn_model* m);
void launch_tracer3(ocn_model* m, double dt, double cn, double cm, int use_m, bool rest);
// levels [zlo, zhi) (-1: Nz), optionally followed by a second run [zlo2, zhi2) of the same length in the same launch
void launch_fused_tend_step(ocn_model* m, double dt, double cn, double cm, int use_m, int zlo = 0, int zhi = -1, int zlo2 = 0, int zhi2 = 0);
void launch_rhs_wrap(ocn_model* m, double dt, double* rhs);
void launch_project(ocn_model* m, double dt, const double* phi, bool store_p = true);
void launch_pressure_images(ocn_model* m, const double* phi);   // pNHS with all periodic images from the compact (Nx, Ny, Nz) phi
void launch_tracer_steps(ocn_model* m, double dt, double cn, double cm, int use_m);
int fused_exchange_ws(ocn_model* m);
int fused_exchange_phi(ocn_model* m, const double* phi);
int poisson_run(ocn_model* m);   // transforms + spectral solve on the solver's rhs buffer, in place

// ---- poisson.hip ------------------------------------------------------------------------------------
PoissonSolver* poisson_create(ocn_model* m);
void poisson_destroy(PoissonSolver* s);
int poisson_solve(ocn_model* m, double dt);             // rhs from velocities -> pNHS interior
int poisson_solve_rhs(ocn_model* m, const double* rhs_dev, double* phi_dev);  // generic (tests)
double* poisson_rhs_buffer(PoissonSolver* s);

// ---- zfft.hip ---------------------------------------------------------------------------------------------
void* zsolve_create(ocn_ctx* ctx, const std::vector<double>& lx_half, const std::vector<double>& ly_local);
void zsolve_destroy(void* z);
void zsolve_run(ocn_ctx* ctx, void* z, void* spec, int Nz, const double* lz, double norm, long zero_col);
void yfft_run(ocn_ctx* ctx, void* z, void* spec, int Nxh, int Ny, int Nz, int inverse);
void xfft_rhs_run(ocn_model* m, void* z, void* spec, double dt, int extra_plane = 0);
// split-y form (Ny = 256): y stage 1 in the x passes, y stage 2 in the z pass; the spectrum between them has the row pitch split_y_pitch
bool split_y_ok(int Nx, int Ny, int Nz);
int split_y_pitch(int Nx);
void xfft_rhs_sy_run(ocn_model* m, void* tw, void* spec, double dt);
void zsolve_sy_run(ocn_ctx* ctx, void* zs, void* spec, int Nx, int Nz, const double* lz, double norm);
void xinv_sy_run(ocn_ctx* ctx, void* tw, const void* spec, double* real, int Nx, int Ny, int Nz);
bool poisson_split_y(const ocn_model* m);       // the split-y form serves the model's pressure solve
bool poisson_local_wstar(const ocn_model* m);   // z-slab runs: the w* term above the slab enters in spectral space, no w* plane exchange
bool fft_size_ok(int n);   // 128, 256, 512: sizes of the custom transform passes
bool zsolve_size_ok(int n);   // those and 320, 384: sizes of the fused z stage
bool poisson_custom_xy(const ocn_model* m);
int poisson_run_from_predictor(ocn_model* m, double dt);   // fused rhs + custom x/y passes (fast path)

// ---- zslab.hip --------------------------------------------------------------------------------------------
void* zslab_create(ocn_ctx* ctx, const std::vector<double>& lx_half, const std::vector<double>& ly, int n, int R, int rank);
void zslab_destroy(void* z);
int zslab_run(ocn_ctx* ctx, void* z, void* spec, double dz2, double scale, const void* below = nullptr, void* phi_below = nullptr);
bool poisson_local_phi_below(const ocn_model* m);
const double* poisson_phi_below(const ocn_model* m);   // that plane, (Nx, Ny), behind the solver's real buffer   // z-slab runs: the pressure plane below the slab is computed by this rank (no exchange)

// ---- comm.hip ---------------------------------------------------------------------------------------------
int comm_exchange(ocn_ctx* c, const std::vector<CommOp>& sends, const std::vector<CommOp>& recvs, hipStream_t st = nullptr);   // st: default the context's stream
int comm_halo_exchange_z(ocn_model* m, Field** fs, int n, hipStream_t st = nullptr);
bool comm_can_overlap(const ocn_ctx* c);   // the transport is stream-ordered on the device (RCCL, or self-copies of a forced one-rank slab run)
int halo_settle(ocn_model* m);             // the model's stream waits for an exchange still in flight (api.hip)
int comm_halo_exchange_y(ocn_model* m, Field** fs, int n);
int comm_alltoall(ocn_ctx* c, const void* send, void* recv, size_t block_bytes);
void comm_destroy(ocn_ctx* c);

// ---- profiling ----------------------------------------------------------------------------------------
struct ProfScope {
  ocn_ctx* c;
  hipEvent_t a = nullptr, b = nullptr;
  const char* name;
  ProfScope(ocn_ctx* ctx, const char* nm);
  ~ProfScope();
};
