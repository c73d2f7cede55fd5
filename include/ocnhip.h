/*
 * ocnhip.h -- C ABI of libocnhip.so: an MI355X (gfx950) implementation of Oceananigans'
 * NonhydrostaticModel `time_step!` hot path on a RectilinearGrid.
 *
 * The reference (Oceananigans.jl v0.76.8) is pure Julia and has no FFI / plugin registry: its only
 * extension point is multiple dispatch on the architecture type carried by the grid
 * (src/Architectures.jl:53-142, src/Grids/grid_utils.jl:39).  A `ROCmGPU <: AbstractArchitecture`
 * shim overloads the phase-level functions listed beside each entry point below
 * and forwards them here with `ccall`.  Paths are relative to /root/reference/src.
 *
 * Conventions
 *   - every function returns 0 (OCN_OK) or a negative OCN_E* code; nothing throws across the boundary;
 *     the message of the last failure is available from ocn_last_error().
 *   - the library owns all device memory behind handles; host buffers belong to the caller and only
 *     need to stay alive for the duration of the (synchronous) upload / download call.
 *   - field memory is the reference's *parent* array: column-major (x fastest), halos included,
 *     size total_size(loc, grid) (Grids/new_data.jl:16-61, Grids/grid_utils.jl:105-128), so a Julia
 *     `OffsetArray` can alias ocn_field_device_ptr() with the usual offsets.  Exception: when x or y is
 *     Bounded or Flat the rows / planes are pitched (like hipMallocPitch: one pitch of N+2H+1 for Face- and
 *     Center-located fields; a Flat x / y direction is stored with broadcast copies).  ocn_field_layout()
 *     returns the element strides and the origin of the logical parent inside the allocation, so the
 *     alias becomes a strided view; ocn_field_upload / download always speak the dense parent layout.
 *   - pointer stability: ocn_field_device_ptr() of u, v, w, pHY', pNHS, nu_e and kappa_e never changes during the life
 *     of a model (every time-stepping path writes the corrected velocities back into the same arrays).  The
 *     tendency sets G^n / G^- and, on the tiled kernels' paths, the tracers are double buffered and ROTATE:
 *     re-query their pointers after every ocn_time_step (tests/test_model_contracts.py asserts both halves).
 *   - when pNHS is current: on a single-rank model of the all-in-one periodic path no time step reads pNHS, so its
 *     projections leave the field alone and the library writes it (interior and every periodic image) from the solver's
 *     buffer when somebody asks: ocn_field_download / get_interior / set_interior(OCN_F_PNHS), ocn_fill_halos with the
 *     pNHS bit, ocn_pressure_correct_velocities, and before ocn_poisson_solve_host / ocn_pressure_correction reuse the
 *     solver's buffers.  Through these calls the field always reads as if every projection had stored it; the price is
 *     one more launch and a second read of the 8 B / cell buffer per request.  ocn_sync does NOT write it.  Asking for
 *     ocn_field_device_ptr(m, OCN_F_PNHS) writes the field and, since the library cannot see reads through the alias,
 *     makes every later projection of that model store it again (ocn_model_path says so); the pointer stays the same.
 *     OCNHIP_EAGER_PRESSURE=1 at model creation stores it in every projection from the start.
 *   - a model that needs wider halos than its grid has (WENO5 / U5: 3) works on a private copy of the grid with the
 *     wider halo, as the reference's with_halo does (nonhydrostatic_model.jl:140-148); the caller's grid and other
 *     models on it are left alone.
 *   - one context = one device + one in-order HIP stream.  Compute calls are asynchronous with
 *     respect to the host and ordered on that stream; only ocn_sync, uploads and downloads block.
 *   - handles are not thread-safe: one host thread per context.
 */
#ifndef OCNHIP_H
#define OCNHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCN_ABI_VERSION 5

/* error codes */
enum {
  OCN_OK = 0,
  OCN_EINVAL = -1,       /* bad argument / unsupported configuration             */
  OCN_ENOMEM = -2,       /* device or host allocation failed                     */
  OCN_EHIP = -3,         /* a HIP / hipFFT / RCCL call failed                    */
  OCN_EUNSUPPORTED = -4, /* valid in the reference, outside this library's scope */
  OCN_ESTATE = -5        /* call made in the wrong state                         */
};

/* topology of one direction (Grids/Grids.jl:60-93) */
enum { OCN_PERIODIC = 0, OCN_BOUNDED = 1, OCN_FLAT = 2 };
/* location of a field along one direction (Grids/Grids.jl: Center, Face) */
enum { OCN_CENTER = 0, OCN_FACE = 1 };
/* advection schemes (Advection/: centered_second_order.jl, centered_fourth_order.jl,
 * upwind_biased_fifth_order.jl, weno_fifth_order.jl:162-180 with zweno = true / false) */
enum { OCN_ADV_NONE = 0, OCN_ADV_C2 = 1, OCN_ADV_C4 = 2, OCN_ADV_U5 = 3, OCN_ADV_WENO5_Z = 4, OCN_ADV_WENO5_JS = 5,
       OCN_ADV_U1 = 6, OCN_ADV_U3 = 7 };   /* upwind_biased_first_order.jl, upwind_biased_third_order.jl (boundary buffer 1) */
/* time steppers (TimeSteppers/quasi_adams_bashforth_2.jl, runge_kutta_3.jl) */
enum { OCN_STEPPER_AB2 = 0, OCN_STEPPER_RK3 = 1 };
/* closures (TurbulenceClosures/turbulence_closure_implementations/{scalar_diffusivity,anisotropic_minimum_dissipation}.jl) */
enum { OCN_CLOSURE_NONE = 0, OCN_CLOSURE_SCALAR = 1, OCN_CLOSURE_AMD = 2 };
/* buoyancy models (BuoyancyModels/buoyancy_tracer.jl:12, linear_equation_of_state.jl:69-77) */
enum { OCN_BUOYANCY_NONE = 0, OCN_BUOYANCY_TRACER = 1, OCN_BUOYANCY_LINEAR_TS = 2 };
/* boundary-condition kinds (BoundaryConditions/boundary_condition.jl:8-11,77-96) */
enum { OCN_BC_DEFAULT = 0, OCN_BC_PERIODIC = 1, OCN_BC_NOFLUX = 2, OCN_BC_FLUX = 3, OCN_BC_VALUE = 4,
       OCN_BC_GRADIENT = 5, OCN_BC_IMPENETRABLE = 6, OCN_BC_NONE = 7 };
/* sides */
enum { OCN_WEST = 0, OCN_EAST = 1, OCN_SOUTH = 2, OCN_NORTH = 3, OCN_BOTTOM = 4, OCN_TOP = 5 };

#define OCN_MAX_TRACERS 8

/* field identifiers inside a model (Fields/field_tuples.jl:133-246) */
enum {
  OCN_F_U = 0, OCN_F_V = 1, OCN_F_W = 2,
  OCN_F_PHY = 3,  /* pHY'  (absent for Flat z)  */
  OCN_F_PNHS = 4, /* pNHS                        */
  OCN_F_GN = 16,  /* G^n : OCN_F_GN + {0,1,2, 3+tracer}   (TimeSteppers: timestepper.G^n) */
  OCN_F_GM = 32,  /* G^- : OCN_F_GM + {0,1,2, 3+tracer}                                    */
  OCN_F_TRACER = 48, /* tracers: OCN_F_TRACER + index                                      */
  OCN_F_NU = 64,     /* AMD eddy viscosity nu_e;  OCN_F_KAPPA + index: kappa_e             */
  OCN_F_KAPPA = 72
};

typedef struct ocn_ctx ocn_ctx;
typedef struct ocn_grid ocn_grid;
typedef struct ocn_model ocn_model;
typedef struct ocn_field ocn_field;   /* a stand-alone field on a grid (ocn_field_create) */

/* RectilinearGrid(size=, halo=, topology=, x=, y=, z=)  -- Grids/rectilinear_grid.jl:249-279.
 * x and y must be regular (extent given); z is regular when z_faces == NULL, otherwise z_faces
 * holds the Nz+1 interior face positions (a "vertically stretched" grid even if the spacing is
 * uniform, which selects the Fourier-tridiagonal solver exactly as NonhydrostaticModels.jl:18-27). */
typedef struct ocn_grid_desc {
  int32_t N[3];        /* Nx, Ny, Nz (1 for Flat directions)              */
  int32_t H[3];        /* halo (0 for Flat directions)                    */
  int32_t topology[3]; /* OCN_PERIODIC / OCN_BOUNDED / OCN_FLAT           */
  double x0[3];        /* left end of the domain per direction            */
  double L[3];         /* extent per direction (ignored for stretched z)  */
  const double* z_faces; /* NULL or Nz+1 doubles (host)                   */
  /* domain decomposition (Distributed/multi_architectures.jl:20-47): N is the GLOBAL size; after ocn_comm_init the
   * library cuts triply periodic grids into z-slabs and (Periodic, Periodic, Bounded) grids into y-slabs and
   * every field of the model has this rank's local shape (ocn_field_shape) */
  int32_t rank, nranks;
} ocn_grid_desc;

/* one side of one field: kind + constant value or host array over the two other (interior) dims */
typedef struct ocn_bc {
  int32_t kind;         /* OCN_BC_*  (OCN_BC_DEFAULT -> field_boundary_conditions.jl:13-35) */
  double value;         /* used when array == NULL                                            */
  const double* array;  /* optional host array (N_a x N_b, column-major), copied at creation */
} ocn_bc;

/* NonhydrostaticModel(; grid, advection, buoyancy, coriolis, closure, boundary_conditions, tracers,
 * timestepper) -- Models/NonhydrostaticModels/nonhydrostatic_model.jl:102-203.  A UniformStokesDrift and forcings without field
 * dependencies (Relaxation, ContinuousForcing) are user functions that the caller evaluates into tables and arrays
 * (ocn_model_create_with, ocn_model_create_forced).  Background fields are user functions too: the caller evaluates them into
 * column tables and parent-layout arrays (ocn_model_create_background).  Forcings with field dependencies, discrete-form and
 * advective forcings, background fields that vary in x or y and in time, immersed boundaries and particles are user Julia
 * closures / out of scope: not representable across a C ABI, the shim rejects them. */
typedef struct ocn_model_desc {
  int32_t advection;   /* OCN_ADV_*                                   */
  int32_t stepper;     /* OCN_STEPPER_*                               */
  double chi;          /* AB2 parameter (quasi_adams_bashforth_2.jl:45: 0.1) */
  int32_t n_tracers;   /* <= OCN_MAX_TRACERS                          */
  int32_t closure;     /* OCN_CLOSURE_*                               */
  double nu;           /* ScalarDiffusivity nu                        */
  double kappa[OCN_MAX_TRACERS]; /* ScalarDiffusivity kappa per tracer */
  double amd_Cnu;      /* AMD Poincare constants                      */
  double amd_Ckappa[OCN_MAX_TRACERS];
  double amd_Cb;       /* AMD buoyancy-modification multiplier (anisotropic_minimum_dissipation.jl:142-154,299-312) */
  int32_t amd_has_Cb;  /* 0: Cb = nothing (the default; the term is skipped), 1: amd_Cb is used */
  int32_t coriolis_fplane; /* 0 / 1 */
  double f;            /* FPlane f (Coriolis/f_plane.jl:42-44)         */
  int32_t buoyancy;    /* OCN_BUOYANCY_*                              */
  int32_t b_index, T_index, S_index; /* tracer indices used by the buoyancy model (-1: absent) */
  double g, alpha, beta; /* SeawaterBuoyancy(LinearEquationOfState)   */
  ocn_bc bcs[3 + OCN_MAX_TRACERS][6]; /* [field: u,v,w,tracers...][side] */
  /* boundary conditions of the AMD diffusivity fields (boundary_conditions = (; nu_e = ..., kappa_e = (; T = ...)) in the
   * reference: nonhydrostatic_model.jl:150-160); OCN_BC_DEFAULT (0) everywhere = the auxiliary-field defaults */
  ocn_bc nu_bcs[6];
  ocn_bc kappa_bcs[OCN_MAX_TRACERS][6];
} ocn_model_desc;

/* ---- context (Architectures.jl:53-142: device, array_type, arch_array, device_event) ---------- */
int ocn_abi_version(void);
int ocn_init(int device_id, ocn_ctx** out);
void ocn_destroy(ocn_ctx* ctx);
int ocn_sync(ocn_ctx* ctx);                       /* wait(device(arch), event) everywhere in the reference.  Slab runs: the
                                                   * halo planes of the last step may still be travelling on the library's
                                                   * communication stream when ocn_time_step returns; ocn_sync, every
                                                   * field accessor and every phase-level call wait for them first */
const char* ocn_last_error(ocn_ctx* ctx);         /* ctx may be NULL: last global error */
void* ocn_stream(ocn_ctx* ctx);                   /* the hipStream_t, for callers that enqueue their own work */

/* ---- grid (Grids/rectilinear_grid.jl:249-279, Grids/zeros.jl:7) --------------------------------- */
int ocn_grid_create(ocn_ctx* ctx, const ocn_grid_desc* desc, ocn_grid** out);
void ocn_grid_destroy(ocn_grid* g);

/* ---- model -------------------------------------------------------------------------------------- */
int ocn_model_create(ocn_grid* g, const ocn_model_desc* desc, ocn_model** out);
/* NonhydrostaticModel(; closure = SmagorinskyLilly(C, Cb, Pr)) -- smagorinsky_lilly.jl:68-69,85-106 -- or the 2-tuple
 * (SmagorinskyLilly, ScalarDiffusivity) of the reference's ocean-LES regression.  Everything but the closure comes from
 * `desc`, whose layout is unchanged: desc->closure is OCN_CLOSURE_NONE (SmagorinskyLilly alone) or OCN_CLOSURE_SCALAR
 * (desc->nu / desc->kappa are the tuple's molecular part; the two flux divergences add).  nu_e is the field OCN_F_NU, filled
 * with desc->nu_bcs; kappa_e of tracer t is nu_e / Pr[t], an operation on nu_e and not a field, so desc->kappa_bcs must be
 * all OCN_BC_DEFAULT.  OCN_EUNSUPPORTED: a Flat direction; OCN_EINVAL: any other desc->closure, a Pr that is zero or not
 * finite, kappa_bcs set. */
typedef struct ocn_smagorinsky_lilly_desc {
  double C;                     /* Smagorinsky constant (0.16)                                            */
  double Cb;                    /* buoyancy multiplier of the stability function (1.0); 0 switches it off */
  double Pr[OCN_MAX_TRACERS];   /* turbulent Prandtl number per tracer (1.0)                              */
} ocn_smagorinsky_lilly_desc;
int ocn_model_create_smagorinsky_lilly(ocn_grid* g, const ocn_model_desc* desc, const ocn_smagorinsky_lilly_desc* smag, ocn_model** out);
/* The general creator (additive: OCN_ABI_VERSION and every struct layout are unchanged).  smag == NULL: as ocn_model_create;
 * else as ocn_model_create_smagorinsky_lilly.  features: OCN_FEATURE_* bits.
 *
 * OCN_FEATURE_STOKES_DRIFT -- NonhydrostaticModel(; stokes_drift = UniformStokesDrift(∂z_uˢ, ∂z_vˢ, ∂t_uˢ, ∂t_vˢ)), StokesDrift.jl:46-80:
 *   G_u += I_xz(w) ∂z_uˢ(z_c, t) + ∂t_uˢ(z_c, t),  G_v += I_yz(w) ∂z_vˢ(z_c, t) + ∂t_vˢ(z_c, t),
 *   G_w -= I_xz(u) ∂z_uˢ(z_f, t) + I_yz(v) ∂z_vˢ(z_f, t).
 * The four functions of (z, t) cannot cross this boundary; the caller evaluates them into tables (ocn_model_set_stokes_drift).  It is
 * a creation-time property because it decides the kernels (never the all-in-one periodic path; ocn_model_path says so).  All
 * tables are zero until set.  OCN_EUNSUPPORTED: Flat z; a distributed grid (z- or y-slabs, more than one rank,
 * OCNHIP_FORCE_DIST). */
#define OCN_FEATURE_STOKES_DRIFT 1u
int ocn_model_create_with(ocn_grid* g, const ocn_model_desc* desc, const ocn_smagorinsky_lilly_desc* smag, uint32_t features, ocn_model** out);
/* Tables of the drift for the tendency evaluation of stage `stage` (0..2; QuasiAdamsBashforth2 uses 0; the kernel-by-kernel
 * verbs read slot `stage of ocn_clock` - 1): ∂z_uˢ, ∂z_vˢ at znode(Center, k), the same two at znode(Face, k), ∂t_uˢ, ∂t_vˢ at
 * znode(Center, k), k = 1..Nz, n = Nz entries each; a NULL table is all zeros (the reference's addzero).  The values are
 * copied before the call returns and uploaded on the model's stream; the device addresses of a slot never change, so a
 * replayed step graph reads whatever was set last.  OCN_ESTATE: a model created without the feature; OCN_EINVAL: stage
 * outside 0..2, n != Nz. */
int ocn_model_set_stokes_drift(ocn_model* m, int stage, const double* dz_us_c, const double* dz_vs_c, const double* dz_us_f,
                               const double* dz_vs_f, const double* dt_us_c, const double* dt_vs_c, int n);
/* clock.time at which each stage of the next ocn_time_step(m, dt, .) computes its tendencies, accumulated exactly as the
 * steppers do (runge_kutta_3.jl:81-152: the clock ticks between stages): *nstages = 1 (AB2) or 3 (RK3). */
int ocn_model_stage_times(const ocn_model* m, double dt, double times[3], int32_t* nstages);
/* NonhydrostaticModel(; forcing = (u = Relaxation(...), T = (Relaxation(...), Forcing(func)), ...)) -- Forcings/relaxation.jl:80-84,
 * continuous_forcing.jl:116-125, multiple_forcings.jl, nonhydrostatic_tendency_kernel_functions.jl:71,128,180,231.  For every
 * forced field phi, at phi's own nodes -- u (Face, Center, Center), v (Center, Face, Center), w (Center, Center, Face k = 1..Nz),
 * tracers at centres -- and with t = clock.time of the stage:
 *     G_phi += sigma (tau - phi) + F
 * sigma = rate * mask(x, y, z) (the caller forms the product), tau = target(x, y, z, t) or a number, F = the sum of the field's
 * ContinuousForcings without field dependencies.  The functions cannot cross this boundary; the caller evaluates them, in one or
 * both of two forms per field:
 *   column form -- sigma, tau, F depend on (z, t): three tables of Nz doubles per field and stage slot, read as wave-uniform
 *     scalars; they may change every stage (ocn_model_set_forcing_column);
 *   field form  -- three (Nx, Ny, Nz) arrays per field, constant in time (ocn_model_set_forcing_field).
 * Bit f of either mask stands for field f: 0, 1, 2 are u, v, w and 3 + t is tracer t.  Forcing is a creation-time property: it
 * decides the kernels (never the all-in-one periodic path; ocn_model_path says so) and allocates the storage whose device
 * addresses never change.  Everything is zero until set.  desc == NULL or both masks zero: exactly ocn_model_create_with.
 * OCN_EINVAL: a bit beyond the model's fields; OCN_EUNSUPPORTED: a distributed grid (z- or y-slabs, more than one rank,
 * OCNHIP_FORCE_DIST).  Flat directions are allowed. */
typedef struct ocn_forcing_desc {
  uint32_t column_fields, field_fields;
} ocn_forcing_desc;
int ocn_model_create_forced(ocn_grid* g, const ocn_model_desc* desc, const ocn_smagorinsky_lilly_desc* smag, uint32_t features,
                            const ocn_forcing_desc* forcing, ocn_model** out);
/* Column-form tables of `field` for the tendency evaluation of stage `stage` (0..2; QuasiAdamsBashforth2 uses 0; the
 * kernel-by-kernel verbs read slot `stage of ocn_clock` - 1): sigma, tau, F at the field's z nodes k = 1..Nz, n = Nz entries
 * each; a NULL table is all zeros.  The values are copied before the call returns and uploaded on the model's stream; the device
 * addresses of a slot never change, so a replayed step graph reads whatever was set last.  OCN_ESTATE: the field was not declared
 * in column_fields; OCN_EINVAL: field or stage out of range, n != Nz. */
int ocn_model_set_forcing_column(ocn_model* m, int field, int stage, const double* sigma, const double* tau, const double* F, int n);
/* Field-form arrays of `field`: sigma, tau, F at the field's nodes i = 1..Nx, j = 1..Ny, k = 1..Nz, column-major (Nx, Ny, Nz); a
 * NULL array is absent (zero: the kernels skip its load; tau is only read next to a sigma).  Synchronises the model's stream,
 * then replaces the arrays; callable between steps.  OCN_ESTATE: the field was not declared in field_fields; OCN_EINVAL: field
 * out of range, (nx, ny, nz) != (Nx, Ny, Nz). */
int ocn_model_set_forcing_field(ocn_model* m, int field, const double* sigma, const double* tau, const double* F, int nx, int ny, int nz);
/* NonhydrostaticModel(; background_fields = (u = U, b = B, ...)) -- Fields/background_fields.jl:5-75,
 * nonhydrostatic_tendency_kernel_functions.jl:61-63,118-120,172-174,226-228, momentum_advection_operators.jl:20-86,
 * tracer_advection_operators.jl:8-35.  With (U, V, W) the background velocities and Phi the background of phi, for u, v, w and
 * every tracer phi, with the model's own advection scheme and boundary buffers and t = clock.time of the stage:
 *     G_phi += - div(adv, (U, V, W), phi) - div(adv, (u, v, w), Phi)
 * The upwind bias follows the advecting velocity: the interpolated background velocity in the first term, the interpolated model
 * velocity in the second.  An absent member is the reference's ZeroField: no background velocity at all -> no first term; no
 * background of phi -> no second term of phi; advection = nothing -> neither.  Nothing else sees the background (closure, buoyancy,
 * Coriolis, pressure, halo fills).  A member is a function evaluated at the nodes of the field it belongs to -- U at (Face, Center,
 * Center), V at (Center, Face, Center), W at (Center, Center, Face), tracers at centres -- INCLUDING the halo nodes, at the
 * extended node coordinates: never wrapped periodically, never filled by boundary conditions.  The functions cannot cross this
 * boundary; the caller evaluates each member in one of two forms:
 *   column form -- the member depends on (z, t): one table per stage slot over the parent levels of its field, Nz + 2 Hz entries
 *     (+ 1 for w with a Bounded z; Hz of ocn_model_halo), read as wave-uniform scalars; it may change every stage
 *     (ocn_model_set_background_column);
 *   field form  -- one array in the layout of the logical parent array of its field (ocn_field_shape's totals), constant in time
 *     (ocn_model_set_background_field).
 * Bit f of either mask stands for member f: 0, 1, 2 are U, V, W and 3 + t is the background of tracer t.  Background fields are
 * a creation-time property: they decide the kernels (never the all-in-one periodic path; ocn_model_path says so) and allocate the
 * storage whose device addresses never change.  Everything is zero until set.  background == NULL or both masks zero: exactly
 * ocn_model_create_forced.  OCN_EINVAL: a bit beyond the model's fields, a member in both masks; OCN_EUNSUPPORTED: a distributed
 * grid (z- or y-slabs, more than one rank, OCNHIP_FORCE_DIST).  Flat directions are allowed. */
typedef struct ocn_background_desc {
  uint32_t column_members, field_members;
} ocn_background_desc;
int ocn_model_create_background(ocn_grid* g, const ocn_model_desc* desc, const ocn_smagorinsky_lilly_desc* smag, uint32_t features,
                                const ocn_forcing_desc* forcing, const ocn_background_desc* background, ocn_model** out);
/* Column-form table of `member` for the tendency evaluation of stage `stage` (0..2; QuasiAdamsBashforth2 uses 0; the
 * kernel-by-kernel verbs read slot `stage of ocn_clock` - 1): the member at the z nodes of every parent level of its field,
 * bottom halo first, n entries.  The values are copied before the call returns and uploaded on the model's stream; the device
 * address of a slot never changes, so a replayed step graph reads whatever was set last.  OCN_ESTATE: the member was not declared
 * in column_members; OCN_EINVAL: member or stage out of range, table NULL, n != the field's parent levels. */
int ocn_model_set_background_column(ocn_model* m, int member, int stage, const double* table, int n);
/* Field-form array of `member`: the member at every node of the logical parent array of its field, column-major (tx, ty, tz) as
 * ocn_field_shape reports the totals; a Flat x / y direction has one entry.  Synchronises the model's stream, then replaces the
 * contents (the device address stays); callable between steps.  OCN_ESTATE: the member was not declared in field_members;
 * OCN_EINVAL: member out of range, array NULL, (tx, ty, tz) != the parent's totals. */
int ocn_model_set_background_field(ocn_model* m, int member, const double* array, int tx, int ty, int tz);
/* Tilted gravity, ConstantCartesianCoriolis and quadratic drag -- what examples/tilted_bottom_boundary_layer.jl needs on top of
 * everything above (BuoyancyModels/buoyancy.jl, g_dot_b.jl, update_hydrostatic_pressure.jl:13,16,
 * nonhydrostatic_tendency_kernel_functions.jl:70,127, Coriolis/constant_cartesian_coriolis.jl:68-79).
 *   has_gravity_vector: Buoyancy(model, gravity_unit_vector = (gx, gy, gz)).  With b the buoyancy of desc->buoyancy at the centre
 *     that has the velocity point's own index (not interpolated, as in the reference): G_u += gx b, G_v += gy b, and pHY' is
 *     integrated from I_z(gz b).  Closures that use d_z b keep the model's plain z gradient.  (0, 0, 1) takes this path too and
 *     changes no bit; the caller validates the unit length.
 *   coriolis_cartesian: the rotation vector (fx, fy, fz) with the non-traditional terms,
 *         G_u -= I_x(fy I_z w - fz I_y v),  G_v -= I_y(fz I_x u - fx I_z w),  G_w -= I_z(fx I_y v - fy I_x u),
 *     instead of desc->coriolis_fplane (the two are exclusive; FPlane keeps its own association of the averages).
 *   drag[f][s]: a quadratic drag as the Flux condition of u (f = 0) or v (f = 1) on the bottom (s = 0) or top (s = 1):
 *         flux = ((-cd) sqrt(U U + V V)) U on u,  ((-cd) sqrt(U U + V V)) V on v,   U = u + u_background, V = v + v_background,
 *     both at the location of the field that carries the condition (its own value; the other component by I_xy, y outside) and
 *     at the boundary-adjacent level k = 1 / Nz, halo values as update_state left them.  It enters like every flux:
 *     G[1] += flux / dz, G[Nz] -= flux / dz.  A function of the model's fields cannot cross this boundary
 *     (FluxBoundaryCondition(f, field_dependencies = ...)); the example's drag is offered by its parameters instead.
 * All of it is a creation-time property: it decides kernels (never the all-in-one periodic path; ocn_model_path says which
 * kernels serve the terms).  tilted == NULL or nothing set: exactly ocn_model_create_background.  OCN_EINVAL: a gravity vector
 * with desc->buoyancy == OCN_BUOYANCY_NONE; coriolis_cartesian together with desc->coriolis_fplane; a drag on a side that is not
 * Bounded in z or whose ocn_bc in desc is already set.  OCN_EUNSUPPORTED: a distributed grid (z- or y-slabs, more than one rank,
 * OCNHIP_FORCE_DIST). */
typedef struct ocn_quadratic_drag {
  int32_t present;
  double cd, u_background, v_background;
} ocn_quadratic_drag;
typedef struct ocn_tilted_desc {
  int32_t has_gravity_vector;
  double gx, gy, gz;
  int32_t coriolis_cartesian;
  double fx, fy, fz;
  ocn_quadratic_drag drag[2][2];   /* [u, v][bottom, top] */
} ocn_tilted_desc;
int ocn_model_create_tilted(ocn_grid* g, const ocn_model_desc* desc, const ocn_smagorinsky_lilly_desc* smag, uint32_t features,
                            const ocn_forcing_desc* forcing, const ocn_background_desc* background, const ocn_tilted_desc* tilted,
                            ocn_model** out);
void ocn_model_destroy(ocn_model* m);
/* which kernels serve this model, and if not the fastest ones, why (e.g. "general kernels: parent arrays of 2 GiB or
 * more exceed the tiled kernels' 32-bit byte offsets").  Writes at most n bytes incl. the terminating 0. */
int ocn_model_path(const ocn_model* m, char* buf, size_t n);
/* Whole-step hipGraphs: models on the general kernels and all-in-one periodic boxes of up to 96^3 cells (not slab-decomposed) replay the
 * launches of a step from a hipGraph once a (dt, stepper state) pair repeats -- the launch train of a small model is
 * latency-bound (time_step! of the reference issues the same ~50 launches from Julia: TimeSteppers/quasi_adams_bashforth_2.jl:70-104).
 * *replays = steps served by a graph so far; *active = 1 while the model may use graphs.  OCNHIP_NO_GRAPH=1 disables. */
int ocn_model_graph_replays(const ocn_model* m, int64_t* replays, int32_t* active);
/* halo actually used (the model inflates it like nonhydrostatic_model.jl:140-148) */
int ocn_model_halo(const ocn_model* m, int32_t H[3]);

/* ---- stand-alone fields: Field{LX,LY,LZ}(grid) / zeros(FT, arch, N...) (Fields/field.jl:16-30, Grids/new_data.jl:16-61,
 * Grids/zeros.jl:7).  A zero-filled parent array, halos included, with the layout a model's own field of that location has
 * on this grid (ocn_field_parent_layout reports strides / origin; dense column-major on (Periodic, Periodic, *) grids).
 * loc*: OCN_CENTER / OCN_FACE.  The grid must outlive the field. */
int ocn_field_create(ocn_grid* g, int locx, int locy, int locz, ocn_field** out);
void ocn_field_destroy(ocn_field* f);
int ocn_field_parent_shape(const ocn_field* f, int32_t total[3], int32_t interior[3], int32_t halo[3]);
int ocn_field_parent_layout(const ocn_field* f, int64_t strides[3], int64_t* origin);
void* ocn_field_parent_ptr(ocn_field* f);                                  /* Julia unsafe_wrap / torch from_blob */
int ocn_field_parent_upload(ocn_field* f, const double* host_parent);      /* logical parent array, column-major  */
int ocn_field_parent_download(const ocn_field* f, double* host_parent);

/* ---- fields: parent arrays incl. halos (Fields/field.jl:16-30; OutputWriters/fetch_output.jl:26) - */
int ocn_field_shape(const ocn_model* m, int field_id, int32_t total[3], int32_t interior[3], int32_t halo[3]);
void* ocn_field_device_ptr(ocn_model* m, int field_id);           /* Julia unsafe_wrap / torch from_blob */
/* element strides (x, y, z) of the device array and the element offset of the logical parent's first entry;
 * strides == (1, T0, T0*T1) and origin == 0 on (Periodic, Periodic, *) grids */
int ocn_field_layout(const ocn_model* m, int field_id, int64_t strides[3], int64_t* origin);
int ocn_field_upload(ocn_model* m, int field_id, const double* host_parent);   /* arch_array(GPU(), a) */
int ocn_field_download(const ocn_model* m, int field_id, double* host_parent); /* arch_array(CPU(), a) */
int ocn_field_set_interior(ocn_model* m, int field_id, const double* host_interior); /* Fields/set!.jl:21-39 */
int ocn_field_get_interior(const ocn_model* m, int field_id, double* host_interior);

/* ---- phase-level entry points (each replaces one overloaded Julia method) ------------------------- */
/* fill_halo_regions!(c, bcs, loc, grid)                      BoundaryConditions/fill_halo_regions.jl:34-46
 * mask: bit f set -> fill field f in {u,v,w,pHY,pNHS} ; bit (8+i) -> tracer i                           */
int ocn_fill_halos(ocn_model* m, uint32_t field_mask);
/* update_state!(model)          Models/NonhydrostaticModels/update_nonhydrostatic_model_state.jl:14-37 */
int ocn_update_state(ocn_model* m);
/* calculate_tendencies!(model)  .../calculate_nonhydrostatic_tendencies.jl:12-36 (interior + boundary) */
int ocn_compute_tendencies(ocn_model* m);
/* ab2_step!(model, dt, chi)     TimeSteppers/quasi_adams_bashforth_2.jl:116-150.  The caller of the phase-level entry
 * points owns the clock (ocn_set_clock): previous_dt decides between Euler and AB2 inside ocn_time_step only. */
int ocn_ab2_step(ocn_model* m, double dt, double chi);
/* rk3_substep!(model, dt, gamma, zeta)  TimeSteppers/runge_kutta_3.jl:161-218 ; has_zeta = 0 for stage 1 */
int ocn_rk3_substep(ocn_model* m, double dt, double gamma, double zeta, int has_zeta);
/* store_tendencies!(model)      TimeSteppers/store_tendencies.jl:14-36 */
int ocn_store_tendencies(ocn_model* m);
/* calculate_pressure_correction!(model, dt)  .../pressure_correction.jl:10-23 (fill, rhs, solve, fill) */
int ocn_pressure_correction(ocn_model* m, double dt);
/* solve!(phi, solver, rhs): Solvers/fft_based_poisson_solver.jl:93-120 or
 * Solvers/fourier_tridiagonal_poisson_solver.jl:74-101 (rhs NOT pre-multiplied by dz).
 * rhs / phi: host arrays (Nx,Ny,Nz), used by the Poisson property tests.                                */
int ocn_poisson_solve_host(ocn_model* m, const double* rhs, double* phi);
/* pressure_correct_velocities!(model, dt)    .../pressure_correction.jl:43-56 */
int ocn_pressure_correct_velocities(ocn_model* m, double dt);
/* set!(model; ...) epilogue: update_state!, unit-dt projection, update_state!
 *                                .../set_nonhydrostatic_model.jl:45-58 */
int ocn_set_epilogue(ocn_model* m, int enforce_incompressibility);
/* time_step!(model, dt; euler)  TimeSteppers/quasi_adams_bashforth_2.jl:70-104 / runge_kutta_3.jl:81-152.
 * Whole sequence enqueued on the stream without host synchronisation.                                   */
int ocn_time_step(ocn_model* m, double dt, int force_euler);
/* model.clock (TimeSteppers/clock.jl:14-18) */
int ocn_clock(const ocn_model* m, double* time, int64_t* iteration, int32_t* stage);
int ocn_set_clock(ocn_model* m, double time, int64_t iteration, double previous_dt);
/* max |div U| over the interior (test helper `divergence!`, test/utils_for_runtests.jl:60-67) */
int ocn_max_abs_divergence(ocn_model* m, double* out);

/* ---- multi-GPU: one process per GPU, RCCL (Distributed/multi_architectures.jl:20-137, halo_communication.jl:68-183,
 * distributed_fft_based_poisson_solver.jl:95-196).  Call ocn_comm_init BEFORE ocn_grid_create: grids created afterwards
 * are cut into z-slabs (triply Periodic) or y-slabs ((Periodic, Periodic, Bounded)); every compute call is then
 * collective and must be issued by all ranks in the same order. ---------------------------------------- */
int ocn_comm_unique_id(void* out128);                                      /* ncclGetUniqueId (128 bytes) */
int ocn_comm_init(ocn_ctx* ctx, int rank, int nranks, const void* unique_id128);
/* Can a communicator of `nranks` form?  A throw-away non-blocking ncclCommInitRankConfig polled against `timeout_s` and
 * aborted: returns on EVERY rank (OCN_OK, RCCL's error, or a time-out) where the blocking ocn_comm_init would leave the
 * healthy ranks waiting for ever for one that failed.  Collective; use a unique id of its own.  (The reference's
 * MPI.Init has no counterpart: an MPI job that loses a rank at start-up is killed by its launcher.)               */
int ocn_comm_probe(ocn_ctx* ctx, int rank, int nranks, const void* unique_id128, double timeout_s);
int ocn_comm_rank(const ocn_ctx* ctx, int* rank, int* nranks);

/* ---- HydrostaticFreeSurfaceModel, first slice: SplitExplicitFreeSurface on a RectilinearGrid or LatitudeLongitudeGrid
 * (BASELINE config 5; Models/HydrostaticFreeSurfaceModels/split_explicit_free_surface.jl, split_explicit_free_surface_kernels.jl,
 * Grids/latitude_longitude_grid.jl).  The 3-D momentum tendencies of that model are not part of this library yet: the caller
 * hands their arrays in (ocn_hfield) exactly as ab2_step_free_surface! receives them from the time stepper. ------------------ */
enum { OCN_NOTHING = 2 };   /* third field location: reduced along that direction (Field{LX, LY, Nothing}, Fields/field.jl:441-449) */
enum { OCN_HGRID_RECTILINEAR = 0, OCN_HGRID_LATLON = 1 };
typedef struct ocn_hgrid ocn_hgrid;     /* the grid as the free surface sees it: sizes, halos, topology, per-row metrics, level thicknesses */
typedef struct ocn_hfield ocn_hfield;   /* a field on it: (Face|Center, Face|Center, Center|Face|Nothing), dense parent array incl. halos     */
typedef struct ocn_sefs ocn_sefs;       /* SplitExplicitFreeSurface(grid; gravitational_acceleration, settings)                            */

/* RectilinearGrid(size, x, y, z, halo, topology) with regular x, y (metres), or
 * LatitudeLongitudeGrid(size, longitude, latitude, z, halo, radius, precompute_metrics = true) with regular longitude / latitude
 * (degrees; latitude_longitude_grid.jl:174-213: pass Periodic for x when the longitude spans 360 degrees, else Bounded; y Bounded).
 * z is Bounded, regular (z_faces == NULL, x0[2] .. x0[2] + L[2]) or given by its Nz + 1 faces. */
typedef struct ocn_hgrid_desc {
  int32_t kind;          /* OCN_HGRID_*                                  */
  int32_t N[3], H[3], topology[3];
  double x0[3], L[3];
  const double* z_faces; /* NULL or Nz + 1 doubles (host)                */
  double radius;         /* lat-lon: sphere radius (<= 0: R_Earth, latitude_longitude_grid.jl:3) */
  int32_t partition;     /* 0: the whole grid on this context.  1: latitude bands (y-slabs) over the context's ranks (ocn_comm_init
                          * first): N, x0, L describe the GLOBAL grid, the handle is rank r's band of N[1] / nranks rows (the role
                          * of Partition(1, R) in the reference's DistributedArch, Distributed/multi_architectures.jl); its fields keep the
                          * Bounded shape, fill_halos exchanges rows with the neighbouring bands.  ocn_hgrid_band reports the rows. */
  int32_t band_overlap;  /* with partition = 1: W > 0 makes the handle the band EXTENDED by W rows towards each neighbouring band (none
                          * towards a wall), as a stand-alone Bounded grid -- what a banded SplitExplicitFreeSurface lives on: it sub-cycles
                          * W substeps on the extended rows (the artificial walls spoil one row per substep from the outside in) and
                          * refreshes the overlap rows from the neighbours.  0: the plain band. */
} ocn_hgrid_desc;
int ocn_hgrid_create(ocn_ctx* ctx, const ocn_hgrid_desc* desc, ocn_hgrid** out);
/* rows of the global grid this handle holds: first row (0-based offset j0) and count; global count; whole grid: 0, Ny, Ny */
int ocn_hgrid_band(const ocn_hgrid* g, int32_t* j0, int32_t* ny_local, int32_t* ny_global);
void ocn_hgrid_destroy(ocn_hgrid* g);
/* metrics and nodes as the grid object holds them (grid.Δxᶠᶜᵃ ... latitude_longitude_grid.jl:418-445; grid.φᵃᶠᵃ ...): which =
 * 0 Δx^fc, 1 Δx^cf, 2 Δy^fc, 3 Δy^cf, 4 Az^cc (per row, first entry = row 1 - Hy), 5 Δz^c (levels 1..Nz), 6 / 7 x nodes Face /
 * Center, 8 / 9 y nodes Face / Center (incl. halos).  Copies min(n, entries) doubles, returns the number of entries. */
int ocn_hgrid_metric(const ocn_hgrid* g, int which, double* host, int n);
/* Field{LX, LY, LZ}(grid), LZ = OCN_CENTER or OCN_NOTHING; zero-filled dense parent array (Grids/new_data.jl:16-61) */
int ocn_hfield_create(ocn_hgrid* g, int locx, int locy, int locz, ocn_hfield** out);
void ocn_hfield_destroy(ocn_hfield* f);
int ocn_hfield_shape(const ocn_hfield* f, int32_t total[3], int32_t interior[3], int32_t halo[3]);
void* ocn_hfield_ptr(ocn_hfield* f);                       /* device pointer of the parent array (Julia: unsafe_wrap)     */
int ocn_hfield_upload(ocn_hfield* f, const double* host_parent);
int ocn_hfield_download(const ocn_hfield* f, double* host_parent);
/* fill_halo_regions!(field) with the default conditions: z (no-flux for Center, faces 1 and Nz + 1 zeroed for a ZFaceField:
 * fill_halo_regions_open.jl:34-39), then x and y (Bounded directions before Periodic ones, fill_halo_regions.jl:76-99) */
int ocn_hfield_fill_halos(ocn_hfield* f);
/* SplitExplicitFreeSurface(grid; gravitational_acceleration, settings = SplitExplicitSettings(substeps))
 * (split_explicit_free_surface.jl:46-60; H^fc, H^cf, H^cc = sum of dz :103-110; uniform weights :137-154) */
int ocn_sefs_create(ocn_hgrid* g, double gravitational_acceleration, int substeps, ocn_sefs** out);
void ocn_sefs_destroy(ocn_sefs* s);
/* the free surface's own fields (owned by it): 0 η, 1 U, 2 V, 3 η̅, 4 U̅, 5 V̅, 6 Gᵁ, 7 Gⱽ, 8 Hᶠᶜ, 9 Hᶜᶠ, 10 Hᶜᶜ */
ocn_hfield* ocn_sefs_field(ocn_sefs* s, int which);
/* SplitExplicitSettings(substeps, velocity_weights, free_surface_weights)  (:130-135) */
int ocn_sefs_set_weights(ocn_sefs* s, int n, const double* velocity_weights, const double* free_surface_weights);
/* split_explicit_free_surface_substep!(η, state, auxiliary, settings, arch, grid, g, Δτ, substep_index)  (kernels.jl:31-58) */
int ocn_sefs_substep(ocn_sefs* s, double dtau, int substep_index);
/* `for substep in first:first+count-1 substep!(...) end` (kernels.jl:154-156).  fused = 1: two launches per substep instead
 * of five; fused = 2: one (eta, U, V double buffered inside the object); fused = 3: four substeps per launch on tiles with a ring
 * of four ghost cells (grids of 64 x 16 cells and more; smaller ones run as 2), the last substep of the train by the one-launch
 * kernel; whichever, the whole train is replayed from a hipGraph and leaves the same bits in every parent array, halos included.
 * 0: the reference's five launches. */
int ocn_sefs_substeps(ocn_sefs* s, double dtau, int first_index, int count, int fused);
int ocn_sefs_graph_replays(const ocn_sefs* s, int64_t* replays);
/* the form the last train of substeps (ocn_sefs_substeps, or the sub-cycle of a time step) took on this grid: 0 the reference's five
 * launches per substep, 1 two launches, 2 one launch, 3 several substeps per launch on tiles with ghost rings; -1 before any train.
 * Read-only: what was asked for is lowered where the grid does not admit it (Bounded x: 0; fewer than 64 x 16 cells: at most 2). */
int ocn_sefs_train_mode(const ocn_sefs* s, int* mode);
/* barotropic_mode!(U, V, grid, u, v) (:76-81): into_forcing == 0 -> state.U, state.V; != 0 -> auxiliary.Gᵁ, Gⱽ */
int ocn_sefs_barotropic_mode(ocn_sefs* s, const ocn_hfield* u, const ocn_hfield* v, int into_forcing);
int ocn_sefs_set_average_to_zero(ocn_sefs* s);             /* (:83-87) */
/* barotropic_split_explicit_corrector!(u, v, free_surface, grid) (:97-113) */
int ocn_sefs_corrector(ocn_sefs* s, ocn_hfield* u, ocn_hfield* v);
/* split_explicit_free_surface_step!(free_surface, model, Δt, χ, velocities_update) (:124-171) given timestepper.Gⁿ.u / .v and
 * G⁻.u / .v: averages reset, barotropic mode of the AB2-combined tendencies, `substeps` substeps of Δτ = 2Δt / substeps,
 * η ← η̅, halos of η filled */
int ocn_sefs_step(ocn_sefs* s, const ocn_hfield* Gn_u, const ocn_hfield* Gn_v, const ocn_hfield* Gm_u, const ocn_hfield* Gm_v,
                  double dt, double chi);

/* ---- HydrostaticFreeSurfaceModel: the AB2 time step around the tendency evaluation (config 5, second slice) --------------
 * time_step!(model::HydrostaticFreeSurfaceModel, dt) (TimeSteppers/quasi_adams_bashforth_2.jl:70-104) is
 *   calculate_tendencies!  ->  ab2_step!  ->  pressure_correct_velocities!  ->  store_tendencies!  ->  update_state!
 * The entry points below are everything after calculate_tendencies!; the caller (until the tendency kernels are in the
 * library too) fills G^n; the closures are those of ocn_hydro_set_closure / ocn_hydro_set_horizontal_closure below; no immersed boundary,
 * flat bottom. */
typedef struct ocn_hydro ocn_hydro;
/* ab2_step_field! (quasi_adams_bashforth_2.jl:158-166): f += dt ((1.5 + chi) G^n - (0.5 + chi) G^-) over the grid's cells */
int ocn_hfield_ab2_step(ocn_hfield* f, const ocn_hfield* Gn, const ocn_hfield* Gm, double dt, double chi);
/* store_field_tendencies! (TimeSteppers/store_tendencies.jl:8-11): G^-[i, j, k] = G^n[i, j, k] over the grid's cells */
int ocn_hfield_store_tendency(ocn_hfield* Gm, const ocn_hfield* Gn);
/* compute_w_from_continuity! (compute_w_from_continuity.jl:31-36): w[1] = 0, w[k] = w[k-1] - dz^c[k-1] div_xy(u, v)[k-1];
 * u, v with filled x / y halos */
int ocn_hydro_compute_w(const ocn_hfield* u, const ocn_hfield* v, ocn_hfield* w);
/* update_hydrostatic_pressure! (Models/NonhydrostaticModels/update_hydrostatic_pressure.jl:10-18) with the buoyancy
 * kind 0: none, 1: BuoyancyTracer (T is b), 2: SeawaterBuoyancy(gravitational_acceleration, LinearEquationOfState(alpha, beta))
 * (BuoyancyModels/linear_equation_of_state.jl:69-71); T, S with filled z halos */
int ocn_hydro_pressure(ocn_hfield* pHY, int buoyancy_kind, double gravitational_acceleration, double thermal_expansion,
                       double haline_contraction, const ocn_hfield* T, const ocn_hfield* S);
typedef struct ocn_hydro_desc {
  ocn_sefs* free_surface;
  ocn_hfield *u, *v, *w, *pHY;                /* (F,C,C), (C,F,C), (C,C,F), (C,C,C)                                   */
  int32_t ntracers;
  ocn_hfield** tracers;                       /* ntracers (C,C,C) fields                                              */
  ocn_hfield **Gn, **Gm;                      /* 2 + ntracers each: u, v, then the tracers in order                   */
  int32_t buoyancy_kind, T_index, S_index;    /* as ocn_hydro_pressure; indices into `tracers`                        */
  double gravitational_acceleration, thermal_expansion, haline_contraction;
} ocn_hydro_desc;
/* binds the model's fields (borrowed: they must outlive the handle) */
int ocn_hydro_create(const ocn_hydro_desc* desc, ocn_hydro** out);
void ocn_hydro_destroy(ocn_hydro* h);
/* update_state!(model) (update_hydrostatic_free_surface_model_state.jl:21-48): halo fills of u, v, eta and the tracers, w from
 * continuity, the hydrostatic pressure, halo fills of w and pHY' */
int ocn_hydro_update_state(ocn_hydro* h);
/* ab2_step!(model, dt, chi) (hydrostatic_free_surface_ab2_step.jl:15-48): barotropic mode of u, v; AB2 steps of u, v, tracers;
 * ocn_sefs_step */
int ocn_hydro_ab2_step(ocn_hydro* h, double dt, double chi);
/* ab2_step!, barotropic correction of u and v (barotropic_pressure_correction.jl:41-47), G^- <- G^n, update_state!.
 * fused = 0 issues the reference's kernels one by one; fused = 1 merges the passes over the 3-D fields (about 28 instead of
 * 40 field sweeps) and leaves the same bits in every field, halos included. */
int ocn_hydro_step_after_tendencies(ocn_hydro* h, double dt, double chi, int fused);

/* ---- third slice: calculate_tendencies! (no forcing or immersed boundary; the closures and flux conditions below) and time_step! ----
 * momentum_advection: 0 nothing, 1 VectorInvariant(scheme = EnstrophyConservingScheme()) -- the default --, 2 EnergyConservingScheme
 *   (Advection/vector_invariant_advection.jl:25-80), 3 WENO5(vector_invariant = VorticityStencil()): the vertical-vorticity term as
 *   transporting velocity times the upwind-biased WENO5 interpolation of zeta (vector_invariant_advection.jl:54-66), halo 3;
 *   4 WENO5(vector_invariant = VelocityStencil()): the same term with the WENO5 weights taken from the averaged smoothness indicators
 *   of the tangential velocities (I_y^f u, I_x^f v) instead of zeta's own (Advection/weno_fifth_order.jl:285-293,405-436), halo 3;
 *   3 and 4 use uniform coefficients and Z weights, and the second-order boundary buffer of a Bounded direction;
 * coriolis: 0 nothing, 1 / 2 HydrostaticSphericalCoriolis(rotation_rate = coriolis_parameter) with the Enstrophy- / Energy-
 *   ConservingScheme (Coriolis/hydrostatic_spherical_coriolis.jl:29-66; LatitudeLongitudeGrid only), 3 FPlane(f = coriolis_parameter);
 * tracer_advection: 0 nothing, 1 CenteredSecondOrder() -- the default; bit-exact against the oracle --, 2 CenteredFourthOrder(),
 *   3 UpwindBiasedFifthOrder(), 4 WENO5() (Z weights, uniform coefficients): flux form with this grid's areas
 *   (tracer_advection_operators.jl:33-37, upwind_biased_advective_fluxes.jl:103-128), second-order inside the boundary buffer of a
 *   Bounded direction (topologically_conditional_interpolation.jl:19-83); halos of 2 / 3 / 3 cells.
 * Defaults of a new handle: 1, 0, 1 -- the reference model's. */
int ocn_hydro_set_physics(ocn_hydro* h, int momentum_advection, int coriolis, double coriolis_parameter, int tracer_advection);
/* momentum_advection = an AbstractAdvectionScheme in flux form: U . grad u = div_Uu, U . grad v = div_Uv
 * (Advection/vector_invariant_advection.jl:100-101, momentum_advection_operators.jl:52-71) in place of the momentum_advection of
 * ocn_hydro_set_physics.  scheme: 0 off (that momentum_advection holds again), 1 CenteredSecondOrder() -- the reference model's own
 * default; bit-exact against the oracle --, 2 CenteredFourthOrder(), 3 UpwindBiasedFirstOrder(), 4 UpwindBiasedThirdOrder(),
 * 5 UpwindBiasedFifthOrder(), 6 WENO5() (Z weights, uniform coefficients); second order inside the boundary buffer of a Bounded
 * direction (topologically_conditional_interpolation.jl:19-83).  A later ocn_hydro_set_physics switches it off again.
 * OCN_EINVAL (text in ocn_last_error) for a scheme outside 0..6, on a LatitudeLongitudeGrid -- flux form is not allowed on curvilinear
 * grids (hydrostatic_free_surface_model.jl:201-210) -- and for halos smaller than the stencils read: 1 cell for schemes 1 and 3,
 * 2 for 2 and 4, 3 for 5 and 6 (a Periodic x needs at least as many cells). */
int ocn_hydro_set_flux_form_momentum_advection(ocn_hydro* h, int scheme);
/* WENO5(grid = grid) on a vertically stretched grid (Advection/weno_fifth_order.jl:182-209,526-539,562-584,740-772): the candidate
 * polynomials of the z reconstructions take their coefficients from coeff_z^aaf -- interp_weights over the faces of
 * with_halo((4, 4, 4), grid), stencils r = -1, 0, 1, 2 at the faces 0 .. Nz + 1, read at the face's own index -- in place of 1/3, 5/6,
 * -1/6, ...; x, y, longitude and latitude are regular on these grids and keep the uniform constants, as do the smoothness indicators
 * (stretched_smoothness = false) and the Z weights.  tracers != 0: for the WENO5 tracer scheme (tracer_advection 4 of
 * ocn_hydro_set_physics), on either grid; momentum != 0: for the flux-form WENO5 momentum scheme (scheme 6 of
 * ocn_hydro_set_flux_form_momentum_advection).  The table is computed on the host by this call.  On a grid whose z is regular (given
 * as an extent) there is no table, as in the reference, and the uniform kernels keep running.  ocn_hydro_set_physics switches both
 * off, ocn_hydro_set_flux_form_momentum_advection the momentum one: ask again after the schemes are set.
 * OCN_EINVAL (text in ocn_last_error) when the corresponding scheme is not WENO5, or with fewer than 3 halo cells. */
int ocn_hydro_set_stretched_weno(ocn_hydro* h, int32_t tracers, int32_t momentum);
/* the table of ocn_hydro_set_stretched_weno, for tests: (Nz + 2) x 4 x 3 doubles, [face 0 .. Nz + 1][r = -1, 0, 1, 2][cell of the
 * stencil], last index fastest.  Copies min(n, entries) doubles and returns the number of entries: 0 while there is no table. */
int ocn_hydro_weno_coefficients(ocn_hydro* h, double* out, int64_t n);
/* closure = VerticalScalarDiffusivity(VerticallyImplicitTimeDiscretization(); nu, kappa = (kappa per tracer)) with constant
 * coefficients: implicit_step! of u, v and every tracer inside ab2_step! (hydrostatic_free_surface_ab2_step.jl:72-85,115-128;
 * TurbulenceClosures/vertically_implicit_diffusion_solver.jl:46-100, Solvers/batched_tridiagonal_solver.jl:89-121); no flux through top
 * and bottom; ntracers must be the handle's; all zeros (the default) switch it off.  Other closures stay on the reference's path. */
int ocn_hydro_set_closure(ocn_hydro* h, double nu, int32_t ntracers, const double* kappa);
/* closure = HorizontalScalarDiffusivity(nu, kappa) (TurbulenceClosures/turbulence_closure_implementations/scalar_diffusivity.jl:101;
 * fluxes abstract_scalar_diffusivity_closure.jl:179-182,205-206) and HorizontalScalarBiharmonicDiffusivity(nu4, kappa4)
 * (scalar_biharmonic_diffusivity.jl:21; fluxes and masks abstract_scalar_biharmonic_diffusivity_closure.jl:46-116), both explicit with
 * constant coefficients, kappa / kappa4 per tracer: their flux divergences are subtracted from G^n of u, v and the tracers by
 * ocn_hydro_calculate_tendencies and ocn_hydro_time_step, G <- G - (Laplacian term + biharmonic term), the reference's rounding for
 * any tuple order of these two and the vertically implicit closure above.  They can be combined with ocn_hydro_set_closure.
 * Zeros (the default) switch a closure off and launch nothing.  OCN_EINVAL for a negative or NaN coefficient, an ntracers that is
 * not the handle's, a Laplacian coefficient with fewer than 1 halo cell in x or y, a biharmonic one with fewer than 2. */
int ocn_hydro_set_horizontal_closure(ocn_hydro* h, double nu, double nu4, int32_t ntracers, const double* kappa, const double* kappa4);
/* Coefficients of the two closures above that follow the grid, and their HorizontalDivergence formulations (hyclosure_var.h).
 * ocn_hydro_set_horizontal_closure with numbers keeps its meaning: it removes every table and sets both formulations back to 0.
 *
 * ocn_hydro_set_horizontal_formulation: the viscous term of the Laplacian-order (order 0) or biharmonic-order (order 1) closure is the
 * Horizontal one (formulation 0: flux_ux = flux_vy = -/+ nu delta, flux_uy = -flux_vx = +/- nu zeta) or the HorizontalDivergence one
 * (formulation 1, HorizontalDivergenceScalarDiffusivity / HorizontalDivergenceScalarBiharmonicDiffusivity: the delta fluxes alone,
 * abstract_scalar_diffusivity_closure.jl:194-196, abstract_scalar_biharmonic_diffusivity_closure.jl:56-57; no tracer flux).  Call it
 * before a setter that takes a closure tuple.  OCN_EINVAL outside 0 / 1.
 *
 * ocn_hydro_set_horizontal_coefficient_table: the coefficient `field` (0 the viscosity, 1 + q the diffusivity of tracer q) of the
 * closure of `order` is zonally uniform and varies with row and level: two tables of nrows x nlevels doubles, entry [r + k * nrows],
 * r the row of the grid's per-row metric arrays (reference row j is r = j - 1 + Hy; nrows = Ny + 2 Hy + 1 of this grid or band) and
 * k = 0 .. Nz - 1 (nlevels = Nz).  `a` holds the coefficient where the reference evaluates it for the first kind of flux, `b` for the
 * second (closure_kernel_operators.jl:108-125): nu at (Center, Center, Center) for the delta fluxes and at (Face, Face, Center) for
 * the zeta fluxes; kappa at (Face, Center, Center) for the x flux and at (Center, Face, Center) for the y flux.  a = b = NULL returns
 * the field to its number.  The field is on while it has tables, whatever its number.  OCN_EINVAL for an order or field out of
 * range, one table without the other, a shape that is not the grid's, too small a halo (1 cell, biharmonic 2), or an entry in a row
 * that can reach a tendency (listed at the definition) that is negative, NaN or infinite. */
int ocn_hydro_set_horizontal_formulation(ocn_hydro* h, int32_t order, int32_t formulation);
int ocn_hydro_set_horizontal_coefficient_table(ocn_hydro* h, int32_t order, int32_t field, const double* a, const double* b, int32_t nrows,
                                               int32_t nlevels);
/* FluxBoundaryCondition on one side (OCN_WEST .. OCN_TOP) of u (field 0), v (field 1) or tracer q (field 2 + q), applied to G^n after
 * the interior tendencies by ocn_hydro_calculate_tendencies / ocn_hydro_time_step (apply_flux_bcs.jl).  kind 0: none (default);
 * 1: the constant `value`; 2: `n` values at `host` (z sides Nx x Ny, x sides Ny x Nz, y sides Nx x Nz of this grid or band,
 * first index fastest), copied to the device; 3: linear drag, flux = -value * field at the boundary cell (z sides only).
 * West / south / bottom: G[1] += (flux A) / V; east / north / top: G[N] -= (flux A) / V, with the face area A and the cell volume V
 * of the field's location.  On latitude bands a south / north condition acts on the band touching that wall only; x sides and z
 * sides take the band's rows.  Fluxes on u and v reach the barotropic forcing through G^n; halo fills and the implicit vertical
 * solve do not change.
 * OCN_EINVAL: a Periodic side, the normal velocity's own wall (u west/east, v south/north), a wrong n, value < 0 for kind 3,
 * a field index out of range.  Calling again replaces the condition; array storage is reused.  A kind-2 call synchronises the
 * context's stream before it copies, so a step already queued reads the previous values: replacing the array between steps is
 * time-varying forcing. */
int ocn_hydro_set_flux_bc(ocn_hydro* h, int32_t field, int32_t side, int32_t kind, double value, const double* host, int64_t n);
/* closure = ConvectiveAdjustmentVerticalDiffusivity(discretization; convective_kappaz, convective_nuz, background_kappaz, background_nuz)
 * (TurbulenceClosures/turbulence_closure_implementations/convective_adjustment_vertical_diffusivity.jl), numbers only.  update_state!
 * (ocn_hydro_update_state and the end of every step) sets its diffusivity fields at faces 1..Nz: kappa = background_kappaz where
 * d_z b >= 0, convective_kappaz elsewhere, nu alike (no buoyancy: d_z b = 0); one kappa serves every tracer.  discretization 0,
 * vertically implicit (the reference's default): ab2_step! solves (1 - dt d_z K d_z) f = f* per column for u and v (nu interpolated
 * to the velocity point) and every tracer (kappa), together with the constant coefficients of ocn_hydro_set_closure; and G^n of u and
 * v gets the interior-face w-shear term -d_z(Az (-nu d_x w)) / V (d_y w for v) whenever a viscosity is non-zero.  discretization 1,
 * explicit: G^n gets -div(-K d_z f) for u, v and the tracers.  The explicit terms are summed with those of
 * ocn_hydro_set_horizontal_closure in the order of the closure tuple: `tuple` lists the kinds of its `ntuple` closures in order
 * (OCN_CLOSURE_*, each at most once; ntuple 0: this closure alone or in front).  A tuple may hold the Horizontal and the
 * HorizontalDivergence closure of one order (kinds 1 and 5, 2 and 6) when at most one of them has a non-zero viscosity: the momentum's
 * term of that order then stands where the closure with the formulation of ocn_hydro_set_horizontal_formulation stands, the tracers'
 * where the Horizontal one does.  All-zero coefficients (the default) switch it off.
 * OCN_EINVAL for a negative, NaN or infinite coefficient, a discretization other than 0 / 1, a grid without a halo cell in z, a tuple
 * with a kind twice (a second convective adjustment) or without this closure. */
enum {
  OCN_CLOSURE_VERTICAL_SCALAR = 0,          /* VerticalScalarDiffusivity (ocn_hydro_set_closure) */
  OCN_CLOSURE_HORIZONTAL_SCALAR = 1,        /* HorizontalScalarDiffusivity */
  OCN_CLOSURE_HORIZONTAL_BIHARMONIC = 2,    /* HorizontalScalarBiharmonicDiffusivity */
  OCN_CLOSURE_CONVECTIVE_ADJUSTMENT = 3,    /* ConvectiveAdjustmentVerticalDiffusivity */
  OCN_CLOSURE_RI_BASED = 4,                 /* RiBasedVerticalDiffusivity */
  OCN_CLOSURE_HORIZONTAL_DIVERGENCE_SCALAR = 5,      /* HorizontalDivergenceScalarDiffusivity: the Laplacian-order term of u and v */
  OCN_CLOSURE_HORIZONTAL_DIVERGENCE_BIHARMONIC = 6   /* HorizontalDivergenceScalarBiharmonicDiffusivity: their biharmonic-order term */
};
int ocn_hydro_set_convective_adjustment(ocn_hydro* h, int32_t discretization, double convective_kappaz, double convective_nuz,
                                        double background_kappaz, double background_nuz, int32_t ntuple, const int32_t* tuple);
/* closure = RiBasedVerticalDiffusivity(discretization; coefficient_z_location, Ri_dependent_tapering, nu0, Ri0nu, Ridnu, kappa0, Ri0kappa,
 * Ridkappa) (TurbulenceClosures/turbulence_closure_implementations/ri_based_vertical_diffusivity.jl), numbers only.  update_state! sets
 * kappa = kappa0 taper(Ri, Ri0kappa, Ridkappa) and nu = nu0 taper(Ri, Ri0nu, Ridnu) at k = 1..Nz, with Ri = N^2 / (d_z u^2 + d_z v^2) at
 * face k (0 where N^2 = 0; +-Inf where N^2 != 0 over zero shear, which every taper maps to exactly 0 or 1) -- at face k for either
 * location, as the reference has it; one kappa serves every tracer.  location 0 Face (the default): (Center, Center, Face) fields, used
 * as CAVD's; 1 Center: (Center, Center, Center) fields, interpolated to the faces (0.5 (K[k-1] + K[k]), after x / y for u / v).
 * tapering 0 PiecewiseLinear, 1 Exponential (the default), 2 HyperbolicTangent.  Discretizations and the closure tuple as for
 * ocn_hydro_set_convective_adjustment; nu0 = kappa0 = 0 switches it off.  OCN_EINVAL for a negative or non-finite nu0 or kappa0, a
 * non-finite Ri0, an Rid <= 0 or non-finite, an unknown location, tapering or discretization, a grid without a halo cell in z, a tuple
 * with a kind twice or without this closure, and a tuple (or a handle) that holds a ConvectiveAdjustmentVerticalDiffusivity too: at
 * most one variable-coefficient vertical closure is on at a time (ocn_hydro_set_convective_adjustment refuses the converse). */
int ocn_hydro_set_ri_based_diffusivity(ocn_hydro* h, int32_t discretization, int32_t location, int32_t tapering, double nu0, double Ri0nu,
                                       double Ridnu, double kappa0, double Ri0kappa, double Ridkappa, int32_t ntuple, const int32_t* tuple);
/* diffusivity_fields of the closure above switched on last: which 0 kappa, 1 nu, fields owned by the handle, (Center, Center, Face) or
 * (Center, Center, Center) for a RiBasedVerticalDiffusivity at Center (parent arrays with halos: x / y halos as the reference's fills
 * leave them; Face: face Nz + 1 and the z halos zero; Center: the first z halo on either side a copy of the level next to it); NULL
 * before either closure was first switched on */
ocn_hfield* ocn_hydro_diffusivity_field(ocn_hydro* h, int32_t which);
/* closure = IsopycnalSkewSymmetricDiffusivity(discretization; kappa_skew, kappa_symmetric, slope_limiter = FluxTapering(max_slope),
 * isopycnal_tensor = SmallSlopeIsopycnalTensor(minimum_bz)) (TurbulenceClosures/turbulence_closure_implementations/
 * isopycnal_skew_symmetric_diffusivity.jl, isopycnal_rotation_tensor_components.jl): Gent-McWilliams plus Redi, on the tracers only.
 * kappa_skew[q] and kappa_symmetric[q] are the numbers of tracer q.  update_state! stores the tapering factor, the slopes and
 * eps_R33; calculate_tendencies! subtracts the divergence of the skew and symmetric fluxes from G^n of every tracer in a pass of its
 * own (after the horizontal closures' pass: next to other explicit closures the sum differs from the reference's tuple sum by
 * round-off); ab2_step! solves (1 - dt d_z K d_z) c = c* per column with K = kappa_symmetric eps_R33 plus the kappa of an implicit
 * ConvectiveAdjustmentVerticalDiffusivity or RiBasedVerticalDiffusivity (Face) that is on, together with the constant of
 * ocn_hydro_set_closure.  NaN and +-Inf arise and propagate as in the reference (its min / max, its 0 / 0 at face 1 and face Nz + 1 of
 * a horizontally uniform state).  `tuple` lists the kinds of the closure tuple (kind 7 exactly once; ntuple 0: this closure alone); the
 * setters of the other closures take their tuple without kind 7.  All-zero kappas switch the closure off and free its fields.
 * discretization 0 only (vertically implicit, the default).  OCN_EUNSUPPORTED, with the reason in ocn_last_error, for discretization 1
 * (the reference's explicit method takes 9 arguments and is called with 10: it cannot run), a model without buoyancy (every slope
 * would be 0 / 0), a RiBasedVerticalDiffusivity at Center or an explicit CAVD / RBVD that is on (their setters refuse the converse).
 * OCN_EINVAL for any other discretization, a negative or non-finite kappa, max_slope or minimum_bz, an ntracers that is not the
 * model's, fewer than 2 halo cells in x, y or z (eps at i + 1 reads b at i + 2; eps at face Nz + 1 reads level Nz + 2), a tuple with an
 * unknown kind, with kind 7 twice (at most one such closure) or without it. */
enum { OCN_CLOSURE_ISOPYCNAL_SKEW_SYMMETRIC = 7 };
int ocn_hydro_set_isopycnal_diffusivity(ocn_hydro* h, int32_t discretization, double max_slope, double minimum_bz, int32_t ntracers,
                                        const double* kappa_skew, const double* kappa_symmetric, int32_t ntuple, const int32_t* tuple);
/* diffusivity_fields of the isopycnal closure: which 0 eps_R33, the tapered 33 component of the rotation tensor, a (Center, Center,
 * Face) field owned by the handle (faces 1..Nz of the grid's columns, x / y halos filled, nothing in z); NULL while the closure is off */
ocn_hfield* ocn_hydro_isopycnal_field(ocn_hydro* h, int32_t which);
/* closure = CATKEVerticalDiffusivity(VerticallyImplicitTimeDiscretization(); CD, mixing_length) (TurbulenceClosures/
 * turbulence_closure_implementations/CATKEVerticalDiffusivities/), the reference's TKE-based boundary-layer scheme.  The tracer
 * e_index is the turbulent kinetic energy e.  update_state! computes K^u, K^c, K^e at faces 1..Nz (nothing is filled in z: face
 * Nz + 1 stays zero) and L^e = -CD sqrt|e| / Iz(l_e) at the centres in one launch; u and v are solved with K^u, the
 * tracers with K^c, e with K^e; G^n of e gets shear production and buoyancy flux; G^n of u and v the w-shear term of a vertically
 * implicit closure.  L^e enters the diagonal of e's solve (1 - dt L - upper - lower) when the closure stands alone (ntuple 0): in a
 * tuple the reference's diagonal has no linear term.  mixing_length: the 25 numbers of MixingLength in the order Cb, Cs, Cbu, Cbc, Cbe,
 * Csu, Csc, Cse, Cdu, Cdc, Cde, CAu, CAc, CAe, CASu, CASc, CASe, CKu-, CKur, CKc-, CKcr, CKe-, CKer, CKRiw, CKRic.  top_buoyancy_flux:
 * the static Q^b(i, j) of the convective length, Nx * Ny numbers of this grid's (band's) columns, or n_flux 0 for zero.  The top flux
 * of e (top_tke_flux) is a condition like any other: set it with ocn_hydro_set_flux_bc.  `tuple` as for
 * ocn_hydro_set_convective_adjustment, with this closure first, where the reference sorts it.  on 0 switches the closure off.
 * OCN_EUNSUPPORTED: discretization 1 (the reference's explicit dissipation silently evaluates to zero), a tuple of more than three
 * closures (no shear_production method beyond three), a tuple or handle with a ConvectiveAdjustmentVerticalDiffusivity,
 * RiBasedVerticalDiffusivity or IsopycnalSkewSymmetricDiffusivity (their setters refuse the converse).  OCN_EINVAL: no tracer e, two
 * CATKEs, a parameter where the reference would compute 0 * Inf or divide by zero (Cb, Cs > 0 with Inf legal; the per-field Cb, Cs,
 * Cdelta, CK-, CKRiw finite and > 0; the others finite and >= 0; CKRic finite), a flux array of another size. */
enum { OCN_CLOSURE_CATKE = 8 };
int ocn_hydro_set_catke(ocn_hydro* h, int32_t on, int32_t discretization, double CD, const double* mixing_length, int32_t e_index,
                        const double* top_buoyancy_flux, int64_t n_flux, int32_t ntuple, const int32_t* tuple);
/* diffusivity_fields of the CATKE closure: which 0 K^u, 1 K^c, 2 K^e ((Center, Center, Face) parents; the x / y halos of K^u as the
 * reference's fills leave them), 3 L^e ((Center, Center, Center)); owned by the handle; NULL before the closure was first switched on */
ocn_hfield* ocn_hydro_catke_field(ocn_hydro* h, int32_t which);
/* calculate_tendencies!(model) (calculate_hydrostatic_free_surface_tendencies.jl:15-160): G^n of u, v and every tracer over the
 * grid's cells, from the state update_state! left (filled halos, w, pHY') */
int ocn_hydro_calculate_tendencies(ocn_hydro* h);
/* time_step!(model, dt; euler) (TimeSteppers/quasi_adams_bashforth_2.jl:70-104): chi = -1/2 and G^- = 0 when euler, else 0.1 */
int ocn_hydro_time_step(ocn_hydro* h, double dt, int euler);

/* ---- ImplicitFreeSurface(solver_method = :PreconditionedConjugateGradient, preconditioner = nothing) ----------------------------
 * (Models/HydrostaticFreeSurfaceModels/implicit_free_surface.jl, pcg_implicit_free_surface_solver.jl, Solvers/
 * preconditioned_conjugate_gradient_solver.jl).  Lives on the whole grid (a model on latitude bands all-gathers ∫ᶻQ and every rank
 * solves the whole 2-D problem).  reltol, abstol >= 0, maxiter >= 0 (the reference's defaults: 1e-7, 0, Nx Ny).  ∫ᶻA is computed once
 * at creation (its halos those of the grid, not the reference's (3, 3, 1): the cells the operator reads agree). */
typedef struct ocn_ifs ocn_ifs;
int ocn_ifs_create(ocn_hgrid* g, double gravitational_acceleration, double reltol, double abstol, int64_t maxiter, ocn_ifs** out);
void ocn_ifs_destroy(ocn_ifs* s);
/* which: 0 η (Center, Center), 1 ∫ᶻQ.u (Face, Center), 2 ∫ᶻQ.v (Center, Face), 3 ∫ᶻ_Axᶠᶜᶜ, 4 ∫ᶻ_Ayᶜᶠᶜ, 5 the right-hand side; owned */
ocn_hfield* ocn_ifs_field(ocn_ifs* s, int which);
/* the iterations of the last solve (solver.iteration) and ‖r‖ at its stop test */
int ocn_ifs_iterations(const ocn_ifs* s, int64_t* iterations, double* residual_norm);
/* implicit_free_surface_step! (implicit_free_surface.jl:125-160) from the velocities u, v of the free surface's grid: fills of u and v,
 * ∫ᶻQ, the right-hand side, the PCG solve for η (initial guess: η), the fill of η.  OCN_ESTATE when ‖r‖ stops being finite. */
int ocn_ifs_step(ocn_ifs* s, ocn_hfield* u, ocn_hfield* v, double dt);
/* the model of ocn_hydro_create on the implicit free surface (desc->free_surface must be NULL): ab2_step! ends with
 * implicit_free_surface_step!, the correction is u -= g Δt ∂x η, v -= g Δt ∂y η; every other entry point works as on the split-explicit
 * free surface */
int ocn_hydro_create_implicit(const ocn_hydro_desc* desc, ocn_ifs* free_surface, ocn_hydro** out);
/* ImplicitFreeSurface(solver_method = :FastFourierTransform) (fft_based_implicit_free_surface_solver.jl, Solvers/
 * fft_based_poisson_solver.jl): the same handle type, solved directly by an eigenfunction expansion in x and y,
 * (∇² - 1 / (g Lz Δt²)) η = (δx ∫ᶻQ.u + δy ∫ᶻQ.v - Az η / Δt) / (g Lz Δt Az).  Needs a rectilinear grid (OCN_EINVAL on a
 * latitude-longitude grid: the reference's ArgumentError), a flat bottom, Periodic or Bounded x and y, and at most 4096 points per
 * direction (a line must fit in LDS; OCN_EINVAL otherwise).  Lengths 2^a 3^b 5^c take a fast transform, every other length a direct
 * O(N²) one.  Every entry point above works on the handle; ocn_ifs_field returns NULL for 3 and 4 (this solver has no ∫ᶻA), and 5 is
 * this solver's right-hand side, which -- unlike the reference's, whose storage the solve overwrites -- is still there after the
 * step; ocn_ifs_iterations reports 0 iterations and a zero residual. */
int ocn_ifs_create_fft(ocn_hgrid* g, double gravitational_acceleration, ocn_ifs** out);
/* method: 0 PCG, 1 FFT; x_path, y_path: 0 the fast transform, 1 the direct one (0 for a PCG handle); any pointer may be NULL */
int ocn_ifs_method(const ocn_ifs* s, int* method, int* x_path, int* y_path);

/* ---- measurement helpers (bench.py) -------------------------------------------------------------- */
/* average device time [ms] of the `n` most recent launches of the named phase, measured with HIP
 * events on the context stream when profiling is enabled */
int ocn_profile_enable(ocn_ctx* ctx, int on);
/* restrict event recording to one phase (NULL / "": all phases).  Every recorded event costs a few microseconds of
 * stream time, so a benchmark that times whole steps records only the phase it reports. */
int ocn_profile_filter(ocn_ctx* ctx, const char* phase);
int ocn_profile_read(ocn_ctx* ctx, const char* phase, double* avg_ms, int64_t* count);
int ocn_profile_reset(ocn_ctx* ctx);
/* measured device-to-device copy rate of this GPU: `reps` stream-ordered copies of `bytes` bytes, timed with HIP events;
 * *bytes_per_s counts bytes read + bytes written (the second roofline denominator of BASELINE.md section 2) */
int ocn_measure_copy_rate(ocn_ctx* ctx, size_t bytes, int reps, double* bytes_per_s);

#ifdef __cplusplus
}
#endif
#endif /* OCNHIP_H */
