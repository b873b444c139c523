/*
 * gapflow_hip.h -- C ABI of libgapflow_hip.so, the MI355X (gfx950) implementation of
 * GaPFlow's explicit time-integration hot path.
 *
 * The reference (hannes-holey/GaPFlow) has no FFI for this path: the boundary is its
 * Python API (GaPFlow/problem.py, GaPFlow/integrate.py).  Every entry point below names
 * the reference code it replaces (paths relative to the reference root).  The host side
 * (gapflow_amd/problem.py, gapflow_amd/integrate.py) binds these with ctypes; see
 * INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success or a negative gpf_status;
 *     nothing throws across the boundary; gpf_last_error() gives the message of the
 *     last failure on the calling thread.
 *   - host arrays are BORROWED for the duration of the call and use the reference's
 *     layout: C-contiguous double[ncomp][Nx+2][Ny+2], one ghost cell per side
 *     (problem.py:122-141).  The library owns all device memory.
 *   - a handle is not thread-safe; all work of a handle is issued on one HIP stream.
 *   - all arithmetic is IEEE binary64 ("f64").
 */
#ifndef GAPFLOW_HIP_H
#define GAPFLOW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpf_handle gpf_handle;

typedef enum {
    GPF_OK = 0,
    GPF_ERR_INVALID = -1,     /* bad argument / unsupported configuration */
    GPF_ERR_HIP = -2,         /* HIP runtime error (message has hipGetErrorString) */
    GPF_ERR_NO_DEVICE = -3,   /* no gfx950 device visible */
    GPF_ERR_SOLVER = -4,      /* rocSOLVER / rocBLAS failure, or matrix not positive definite */
    GPF_ERR_STATE = -5        /* call sequence error (e.g. step before upload) */
} gpf_status;

/* Equation of state ids (GaPFlow/models/pressure.py:51-71) */
enum { GPF_EOS_DH = 0, GPF_EOS_PL = 1, GPF_EOS_VDW = 2, GPF_EOS_MT = 3,
       GPF_EOS_CUBIC = 4, GPF_EOS_BWR = 5, GPF_EOS_BAYADA = 6 };

/* Ghost-cell rule per component (GaPFlow/problem.py:676-768) */
enum { GPF_BC_PERIODIC = 0, GPF_BC_DIRICHLET = 1, GPF_BC_NEUMANN = 2 };

/* Piezo-viscosity laws (GaPFlow/models/viscosity.py:34-66) */
enum { GPF_PIEZO_NONE = 0, GPF_PIEZO_BARUS = 1, GPF_PIEZO_ROELANDS = 2,
       GPF_PIEZO_DUKLER = 3, GPF_PIEZO_MCADAMS = 4 };

/* Shear-thinning laws (GaPFlow/models/viscosity.py:69-96) */
enum { GPF_THINNING_NONE = 0, GPF_THINNING_EYRING = 1, GPF_THINNING_CARREAU = 2 };

/* Field ids for gpf_upload / gpf_download */
enum {
    GPF_FIELD_Q = 0,          /* 3 comps: rho, jx, jy                 (problem.py:128)          */
    GPF_FIELD_TOPO = 1,       /* 3 comps: h, dh/dx, dh/dy             (topography.py:252-254)   */
    GPF_FIELD_EXTRA = 2,      /* 1 comp : slip length Ls              (problem.py:132-135)      */
    GPF_FIELD_PRESSURE = 3,   /* 1 comp : derived, stress.py:600-622                            */
    GPF_FIELD_TAU_AVG = 4,    /* 3 comps: xx, yy, xy, stress.py:427-459                         */
    GPF_FIELD_WALL_LOWER = 5, /* 6 comps Voigt = wall_stress_xz.lower + wall_stress_yz.lower    */
    GPF_FIELD_WALL_UPPER = 6, /* 6 comps Voigt (problem.py:554-555)                             */
    GPF_FIELD_PRESSURE_VAR = 7,   /* GP predictive variances (stress.py:97, 499), 1 comp each         */
    GPF_FIELD_WALL_XZ_VAR = 8,
    GPF_FIELD_WALL_YZ_VAR = 9,
    GPF_FIELD_DEFORMATION = 10  /* 1: elastic displacement added to the undeformed gap height (download only) */
};

/*
 * Static description of one problem (or of one x-slab of it).  Mirrors the sanitised
 * dicts of GaPFlow/io.py:128-394 after the host has resolved the boundary-condition
 * side quirks of problem.py:736-754 into "rule and target of each ghost edge".
 */
typedef struct {
    int32_t Nx, Ny;            /* interior cells of this slab; arrays are (Nx+2) x (Ny+2)          */
    double  dx, dy;
    double  U, V;              /* wall velocities, geometry dict                                    */
    double  eta, zeta;         /* shear / bulk viscosity, properties dict                           */
    int32_t eos;               /* GPF_EOS_*                                                         */
    double  eos_par[8];        /* DH: rho0,P0,C1,C2 | PL: rho0,P0,alpha | vdW: M,T,a,b |
                                  MT: rho0,P0,K,n | cubic: a,b,c,d | BWR: T,gamma |
                                  Bayada: rho_l,rho_v,c_l,c_v                                        */
    int32_t piezo;             /* GPF_PIEZO_*                                                       */
    double  piezo_par[4];      /* Barus: aB | Roelands: mu_inf,p_ref,z | Dukler/McAdams: eta_v,rho_l,rho_v */
    /* ghost edges: [0]=ix=0, [1]=ix=Nx+1, [2]=iy=0, [3]=iy=Ny+1; rule per component            */
    int32_t bc_rule[4][3];
    double  bc_value[4];       /* Dirichlet target of that edge (one scalar per edge)              */
    int32_t halo_lo, halo_hi;  /* kind of the rows ix=0 / ix=Nx+1 of this slab:
                                  0 physical ghost row (rule above applied locally),
                                  1 slab halo = copy of a neighbour's interior row (caller's exchange),
                                  2 periodic seam = the domain's periodic ghost row, filled by the
                                    caller's ring exchange instead of a local copy                    */
    /* time stepping (io.py:381-394, problem.py:412-443) */
    int32_t adaptive;
    double  CFL, dt_fixed, tol;
    int64_t max_it;
    int32_t mc_order;          /* +1, -1, or 0 = alternate by step parity (problem.py:521-522)     */
    int32_t device;            /* HIP device ordinal                                                */
    int32_t thinning;          /* GPF_THINNING_*; only the stage-wise step supports it (needs grad p)  */
    double  thinning_par[4];   /* Eyring: tauE | Carreau: mu_inf, lam, a, N                            */
} gpf_config;

/* Per-step scalars (problem.py:334-362, 571-586).  All sums/maxima run over the whole
 * array including ghost cells, as in the reference. */
typedef struct {
    int64_t step;
    double  simtime, dt;       /* dt = step size the NEXT step will use                             */
    double  ekin, ekin_old;    /* Ekin = sum (jx^2+jy^2)/rho/2                                      */
    double  residual;          /* |Ekin-Ekin_old|/Ekin_old/cfl                                      */
    double  v_max, v_sound;    /* max sqrt((jx^2+jy^2)/rho) (sic), max c(rho)                       */
    double  mass;              /* sum rho*h*dx*dy; filled by gpf_scalars only                       */
    int32_t invalid;           /* 1: NaN, 2: negative density (problem.py:319-332)                 */
    int32_t converged;         /* all of the last <=5 residuals < tol (problem.py:359-362)          */
} gpf_scalars_t;

/* ---- lifetime -------------------------------------------------------------------------- */
int gpf_create(const gpf_config* cfg, gpf_handle** out);      /* Problem.__init__, problem.py:77-151 */
int gpf_destroy(gpf_handle* h);
int gpf_set_stream(gpf_handle* h, void* hip_stream);          /* default: the null stream           */
const char* gpf_last_error(void);
int gpf_device_count(void);

/* ---- fields ---------------------------------------------------------------------------- */
int gpf_upload(gpf_handle* h, int field, const double* host, size_t count);     /* count = ncomp*(Nx+2)*(Ny+2) */
int gpf_download(gpf_handle* h, int field, double* host, size_t count);
/* Pressure/WallStress/BulkStress.update without time stepping: refreshes the derived
 * fields from the current q (stress.py:289-362, 427-459, 600-622). */
int gpf_update_closures(gpf_handle* h);

/* ---- time stepping --------------------------------------------------------------------- */
/* _pre_run (problem.py:412-443): step=0, residual=1, dt = CFL*dt_crit or dt_fixed, Ekin_old from q. */
int gpf_pre_run(gpf_handle* h);
/* n calls of Problem.update() (problem.py:509-586) enqueued back-to-back with no host
 * round trip.  If honor_stop != 0 the steps become no-ops on the device once `converged`
 * holds or step == max_it (the `while` of run(), problem.py:401); an invalid state
 * (NaN / rho<0) always rolls back to the pre-step field and stops (problem.py:565-610).
 * log (may be NULL): receives one gpf_scalars_t per executed step, at most log_capacity. */
int gpf_step(gpf_handle* h, int64_t n, int honor_stop, gpf_scalars_t* log, int64_t log_capacity,
             int64_t* n_executed);
/* Measurement aid: n updates with a HIP event pair around each launch of the fused step kernel
 * (recorded on the handle's stream).  *kernel_ms = sum of the n kernel durations, *total_ms =
 * elapsed device time of the whole sequence (stage-1 ghost data, fused step, ghost fill with the commit). */
int gpf_step_timed(gpf_handle* h, int64_t n, double* kernel_ms, double* total_ms);
/* How the fused step of this handle is laid out on the chip (row chunks per strip = waves per SIMD, cache policy of the stores)
 * and how that was decided: grids of a million cells and more time the candidates once on their own data before the first step
 * (GPF_PLAN_TUNE=0: rule of thumb; GPF_CHUNKS / GPF_NT_STORES pin a choice).  Empty until the first step has been planned.
 * The choice changes the order in which the kinetic energy is summed (last bits of the residual), nothing else. */
const char* gpf_plan_note(gpf_handle* h);
/* The closure coefficients of an x-only gap, one record of 8 doubles (A, B, C, S0, S1a, S1b, S2a, S2b: closures.hpp, RowCoef) per
 * row ix = 0 .. Nx+1, then two per x edge for the rows across a periodic slab seam (zero where there is none): count = 8 (Nx+2+4).
 * source 0: the table the fused step reads (built on the device at every upload of the gap and by gpf_set_seam_topo);
 * source 1: the same function evaluated now, row by row, on column 1 of the handle's gap PLANES and on its seam rows.
 * GPF_ERR_STATE unless the handle holds a table: the gap varies along x only, no slip-length field or piezo-viscosity, and
 * GPF_ROWCOEF_TABLE was not 0 at gpf_create (the step kernel then evaluates the coefficients itself, as before the table). */
int gpf_row_coefficients(gpf_handle* h, int source, double* host, size_t count);
/* Which instantiation of the fused step kernel the handle's last step launched: out = {eos, has_ls, piezo, D, topo} -- the
 * equation of state (gpf_config.eos), whether it reads a slip-length field, whether the viscosity is piezo-viscous, the sweep
 * direction of the predictor (+1 / -1) and the gap's form (0 planes, 1 profile over ix, 2 profile over iy, 3 profile over ix with
 * dh/dy = 0, 4: 3 with the row coefficients from the table).  These are the very values the launch selected its kernel with,
 * recorded as it did.  GPF_ERR_STATE before the first such launch (problems that fit one workgroup never make one). */
int gpf_step_variant(gpf_handle* h, int out[5]);
/* The reference-ordered, unfused stage pipeline (closures -> flux -> source -> axpy -> ghost),
 * one kernel per reference function; same results as gpf_step(h,1,...).  Kept for
 * cross-checking and for _finalize (problem.py:588-610). */
int gpf_step_unfused(gpf_handle* h);
/* scalars of the current state (mass, kinetic_energy, v_max, v_sound, dt_crit inputs) */
int gpf_scalars(gpf_handle* h, gpf_scalars_t* out);
int gpf_set_ekin_old(gpf_handle* h, double value);            /* kinetic_energy_old setter, tests/test_wave_decay.py:102 */
int gpf_set_dt(gpf_handle* h, double dt);

/* ---- slab decomposition (one process per GPU, x-slabs) ------------------------------------ */
/* One message per slab and step feeds a SINGLE all-gather: *message (device, *count = 6*pitch + 8 doubles) =
 * [first interior row | last interior row | 8-double record] of the field the current step has produced, where a
 * row is 3 components x the padded row and the record is [sum Ekin, max v^2, max c^2 (NaN as +inf), invalid flags,
 * 0...].  The address is fixed for the life of the handle (usable as an RCCL / torch.distributed buffer).
 *
 * gpf_step_local : stage-1 ghost data + fused stencil + local ghost rules + the message.
 * (caller)       : all-gather the messages of all slabs, rank order, into `gathered` (device, nranks * count).
 * gpf_step_commit: scatter the neighbours' rows into rows ix=0 / ix=Nx+1 (rank_lo: the rank whose LAST row is my
 *                  row 0, rank_hi: the rank whose FIRST row is my row Nx+1, -1 = physical edge), reduce the records
 *                  in rank order and advance dt / residual / step exactly as gpf_step does.
 * Everything is enqueued on the handle's stream; neither call synchronises with the host. */
int gpf_slab_message(gpf_handle* h, void** message, size_t* count);
int gpf_step_local(gpf_handle* h, int honor_stop);
int gpf_step_commit(gpf_handle* h, int honor_stop, const void* gathered, int nranks, int rank_lo, int rank_hi);
/* Elastic deformation of the gap under the film pressure (Topography.update, topography.py:257-280; ElasticDeformation,
 * topography.py:327-437).  gpf_elastic_setup receives the half-space Green's function in Fourier space on a px x py
 * transform grid (px >= Nx+2, py >= Ny+2; doubled along non-periodic axes), as numpy's rfft2 lays it out:
 * greens_ri[px][py/2+1][2] (real, imaginary), count = 2 px (py/2+1); alpha = under-relaxation factor; force_scale =
 * (force per cell / pressure) / (cell area the Green's function is normalised to); relative != 0: pressure and
 * displacement are taken relative to cell [0, 0] (every case but the fully periodic one).  The handle's current
 * topography is kept as the undeformed one.  gpf_elastic_update convolves the pressure of the last closure evaluation,
 * under-relaxes, and rewrites h, dh/dx, dh/dy (np.gradient stencil) in place; GPF_FIELD_DEFORMATION downloads the
 * displacement.  Undivided problems; slabs use gpf_elastic_slab_* below. */
int gpf_elastic_setup(gpf_handle* h, int px, int py, const double* greens_ri, size_t count, double alpha,
                      double force_scale, int relative);
int gpf_elastic_update(gpf_handle* h);
/* The same deformation on an x-slab (topography.py:257-280, 404-437 as a distributed transform; no rank holds the whole
 * spectrum).  gpf_elastic_slab_setup takes this rank's plan (gapflow_amd/elastic.py: SlabElasticPlan; layout in
 * csrc/api_slab_elastic.inc): transform rows it owns, its ky column slab of [0, py/2], the rows it gets back (its rows and
 * one more on each side, plus three seam rows on a periodic seam edge) and every rank's return rows; greens_ri = its slab
 * of the Green's spectrum [px][nk][2]; h0_rows = the undeformed gap of its return rows [nret][Ny+2].  Per step, after
 * gpf_close_step_commit of a valid step:
 *   gpf_elastic_slab_forward   forces of the owned rows (p_ref from rank 0's record in `gathered`), D2Z, column pack
 *   -- all-to-all of buffer 0 into buffer 1 (caller) --
 *   gpf_elastic_slab_convolve  x-transforms, Green's multiply, inverse x-transforms, row pack
 *   -- all-to-all of buffer 2 into buffer 3 (caller) --
 *   gpf_elastic_slab_finish    unpack, Z2D, under-relaxation; reference displacement into buffer 4
 *   -- relative mode: all-gather of buffer 4 into buffer 5 (caller) --
 *   gpf_elastic_slab_apply     h, dh/dx, dh/dy and the displacement of the slab's rows and of its seam block
 * gpf_elastic_slab_buffer returns those device buffers (count in doubles).  Every call only enqueues on the handle's stream. */
int gpf_elastic_slab_setup(gpf_handle* h, int px, int py, int nranks, const int32_t* plan, size_t plan_count,
                           const double* greens_ri, size_t greens_count, const double* h0_rows, size_t h0_count,
                           double alpha, double force_scale, int relative);
int gpf_elastic_slab_buffer(gpf_handle* h, int which, void** ptr, size_t* count);
int gpf_elastic_slab_forward(gpf_handle* h, const void* gathered, int nranks);
int gpf_elastic_slab_convolve(gpf_handle* h);
int gpf_elastic_slab_finish(gpf_handle* h);
int gpf_elastic_slab_apply(gpf_handle* h);

/* Peer-to-peer slab transport (GPUs of one node, one process each).  Instead of a collective library the step's own
 * kernels store the two boundary rows and the 64-byte record straight into the peers' mailboxes (device memory mapped
 * through HIP IPC, xGMI underneath) and the receiving kernel polls a sequence flag -- no host and no extra launches
 * between steps, so gpf_step_p2p(n) enqueues n complete steps at once.
 *   gpf_p2p_export   allocate this slab's mailbox, return its 64-byte IPC handle (exchange them with any transport)
 *   gpf_p2p_connect  map every rank's mailbox; ipc_handles = nranks x 64 bytes in rank order
 *   gpf_step_p2p     n steps; a peer that stays silent for 30 s marks the state invalid (gpf_state: invalid == 3) --
 *                    decided once per launch: every block reports, the last one to arrive stops the handle if ANY block
 *                    missed a flag (no commit, no sequence advance), so a flag that lands at the deadline cannot split
 *                    the blocks of one launch
 *   gpf_p2p_set_timeout   the bound on that wait, in seconds (tests use a fraction of a second)
 * rank_lo / rank_hi as in gpf_step_commit. */
int gpf_p2p_export(gpf_handle* h, void* ipc_handle, size_t handle_bytes);
int gpf_p2p_connect(gpf_handle* h, int rank, int nranks, const void* ipc_handles, int rank_lo, int rank_hi);
int gpf_step_p2p(gpf_handle* h, int64_t n, int honor_stop);
int gpf_p2p_set_timeout(gpf_handle* h, double seconds);
/* Stage-wise step of a slab (GP closures, shear thinning): after each gpf_stage_advance the rows a neighbour needs
 * are packed from the working field (gpf_stage_message -> the same message buffer), all-gathered by the caller and
 * scattered (gpf_stage_absorb); gpf_close_step_local averages, applies the local ghost rules and leaves this slab's
 * record in the message, gpf_close_step_commit reduces the gathered records and advances dt / residual / step. */
/* Shear thinning (stress.py:170-192: eta depends on np.gradient(p)) gives the step a two-row reach in x: the viscosity of a
 * slab's halo row needs the pressure one row further into the neighbour.  With cfg.thinning != 0 the stage messages carry
 * two more rows (density of the second and second-to-last owned row; message length 8*pitch + 8) and the library keeps the
 * neighbours' copies; gpf_upload_beyond seeds them for the initial state (side 0: beyond row 0, 1: beyond row Nx+1;
 * Ny+2 densities).  Only the stage-wise calls serve such a slab (gpf_step_local / gpf_step_p2p refuse it). */
int gpf_upload_beyond(gpf_handle* h, int side, const double* rho_row, size_t count);
int gpf_stage_message(gpf_handle* h);
int gpf_stage_absorb(gpf_handle* h, const void* gathered, int nranks, int rank_lo, int rank_hi);
int gpf_close_step_local(gpf_handle* h);
int gpf_close_step_commit(gpf_handle* h, const void* gathered, int nranks, gpf_scalars_t* out);
/* Read back the run state after a batch of split steps (synchronises). */
int gpf_state(gpf_handle* h, gpf_scalars_t* out);
/* Topography across a periodic seam (halo kind 2): the rows the far side's first interior cell and
 * its upwind neighbour see, needed to reproduce problem.py:683/690 exactly.
 * side 0: edge ix=0, host = topo+Ls of global rows (Nx, Nx+1); side 1: edge ix=Nx+1, rows (1, 0).
 * Layout double[2][4][Ny+2] (h, dh/dx, dh/dy, Ls per row). */
int gpf_set_seam_topo(gpf_handle* h, int side, const double* host, size_t count);

/* ---- stateless operators: GaPFlow/integrate.py ------------------------------------------ */
/* predictor_corrector(q,p,tau,direction) -> flux_x, flux_y   (integrate.py:38-77) */
int gpf_predictor_corrector(int nx, int ny, const double* q, const double* p, const double* tau,
                            int direction, double* flux_x, double* flux_y);
/* source(q,h,stress,stress_lower,stress_upper) -> out        (integrate.py:80-130); h = first 3 comps of the topography */
int gpf_source(int nx, int ny, const double* q, const double* h, const double* stress,
               const double* lower, const double* upper, double* out);

/* ---- stateless operators: GaPFlow/models as functions of arrays ----------------------------------- */
/* stress_bottom / stress_top / stress_avg (models/viscous.py:37, 281, 612) for n points in one call.  Arrays are
 * component-major: q, hh (h, dh/dx, dh/dy), dqx, dqy [3][n] (dqx, dqy may be NULL = zero gradients, the solver's
 * case); eta, Ls [n] (viscosity and slip length per point).  slip_both = 0: slip="top" (only the upper wall slips,
 * what the solver uses); 1: the other branch of viscous.py (both walls; Ls = 0 is no slip).  Outputs, any of which
 * may be NULL: bottom, top [6][n] in Voigt order xx, yy, zz, yz, xz, xy; avg [3][n] = xx, yy, xy. */
int gpf_viscous_stress(int64_t n, const double* q, const double* hh, const double* dqx, const double* dqy,
                       const double* eta, const double* Ls, double U, double V, double zeta, int slip_both,
                       double* bottom, double* top, double* avg);
/* eos_pressure (models/pressure.py:35-76) and eos_sound_velocity (models/sound.py) of n densities; eos / eos_par as
 * in gpf_config; either output may be NULL. */
int gpf_eos(int eos, const double* eos_par, int64_t n, const double* rho, double* pressure, double* sound);
/* models/viscosity.py for n points.  kind 0: piezoviscosity(a0 = pressure, or density for the mixture laws; mu0;
 * law = gpf_config.piezo, par = piezo_par) (viscosity.py:34-66); kind 1: shear_thinning_factor(a0 = shear rate; mu0;
 * law = gpf_config.thinning, par = thinning_par) = mu/mu0 (viscosity.py:69-96); kind 2: shear_rate_avg(a0 = dp/dx,
 * a1 = dp/dy, a2 = h; wall speeds u1, u2; viscosity mu0) (viscosity.py:110-141; law, par unused). */
int gpf_viscosity(int kind, int law, const double* par, double mu0, int64_t n, const double* a0, const double* a1,
                  const double* a2, double u1, double u2, double* out);

/* ---- the unfused step in pieces ------------------------------------------------------------- */
/* For closures that need the host between stages (GP surrogates with active learning, gp.py:435-506):
 * gpf_open_step copies q0; per stage gpf_stage_closures evaluates Pressure/WallStress/BulkStress on the
 * working field (fixed-form laws, then the mean of every GP model that is set), gpf_stage_advance applies
 * flux + source + ghost rules (problem.py:543-560); gpf_close_step averages, checks validity, updates
 * dt / residual (problem.py:563-586).  gpf_step_unfused is exactly open, 2 x (closures, advance), close. */
int gpf_open_step(gpf_handle* h);
int gpf_stage_closures(gpf_handle* h);
int gpf_stage_advance(gpf_handle* h, int stage);
int gpf_close_step(gpf_handle* h, gpf_scalars_t* out);

/* ---- GP surrogate closure: GaPFlow/models/gp.py, models/stress.py ------------------------------ */
/* Stateless fit: K = A (1 + sqrt3 r) exp(-sqrt3 r) + sigma^2 I with r = ||inv_scale o (x - x')||
 * (gp.py:598-603; tinygp GaussianProcess(kernel, X, diag=yerr^2)), Cholesky K = L L^T and alpha = K^-1 Y
 * on the device: rocSOLVER's dpotrf / dpotrs (the copy that lies beside the rocBLAS the process uses); with GPF_USE_ROCSOLVER=0,
 * or where there is no such copy, the library's own blocked Cholesky.  Xn [n][d] and Yn [n][m] row-major, already normalised.  Outputs (host,
 * each may be NULL): L [n][n] row-major lower factor, alpha [n][m], logdet = log det K. */
/* Which factorisation serves this process: "rocsolver_dpotrf", "in-library blocked Cholesky", or the reason neither is available. */
const char* gpf_gp_factorisation(void);
int gpf_gp_fit(int device, int n, int d, int m, const double* Xn, const double* Yn, double amp,
               const double* inv_scale, double sigma, double* L, double* alpha, double* logdet);
/* Attach / replace a surrogate of this problem: which = 0 pressure (m = 1; writes the pressure field),
 * 1 wall shear xz, 2 wall shear yz (m = 2: lower, upper wall; Voigt index 4 / 3, stress.py:91, 356-357).
 * dims[d]: feature index of each active dimension in [rho, jx, jy, h, dh/dx, dh/dy, extra]
 * (gp.py:223-232); x_scale[d]: the database normalisers of those features (db.py:264-266);
 * yscale: output scale (stress.py:230-242, 562-564).  The model is factorised on the device. */
int gpf_gp_set_model(gpf_handle* h, int which, int n, int d, int m, const int32_t* dims, const double* x_scale,
                     const double* Xn, const double* Yn, double amp, const double* inv_scale, double sigma,
                     double yscale);
int gpf_gp_clear_model(gpf_handle* h, int which);
/* The reference normalises test inputs and outputs with the database's CURRENT max-abs scales (properties Xtest / Yscale,
 * stress.py:195-242, 542-564) while the factorised model and its cached alpha are those of the last fit (gp.py:343-349):
 * after the database has grown through another model and before this model's next fit, the mean is
 * Ks(x / x_scale_now)^T alpha_fit * yscale_now and the variance alike; the GP sound speed re-solves alpha from
 * Y_raw / yscale_now (stress.py:588, 533-535), so there only x_scale changes.  This call hands the current scales to an
 * attached model without refitting it. */
int gpf_gp_set_scales(gpf_handle* h, int which, const double* x_scale, double yscale);
/* Predictive variance A - ||L^-1 k(X, x*)||^2 (gp.py:509-522) of model `which` at every cell, written to
 * the GPF_FIELD_*_VAR field (times yscale^2); *max_var = its maximum (the active-learning criterion,
 * gp.py:408).  on_open_step != 0: evaluate on the working field of an open step. */
int gpf_gp_variance(gpf_handle* h, int which, int on_open_step, double* max_var);
/* Posterior-mean passes over the grid since gpf_create: launched[which] per model, and *reused = evaluations of the
 * pressure surrogate that were served by the pass that closed the previous step (stress.py:533-537 evaluates the
 * sound speed -- the slope of the mean -- on the state the next step's first closure update, stress.py:522-531, sees
 * again: one kernel launch yields both).  Introspection for tests and bench.py; GPF_GP_NO_STATE_MEAN=1 at gpf_create
 * turns the reuse off. */
int gpf_gp_pass_counts(gpf_handle* h, int64_t launched[3], int64_t* reused);

/* Hyper-parameter training on the device (replaces what tinygp + jax.grad + jaxopt evaluate per optimiser step,
 * gp.py:290-335, 576-603): -log p(Y | X, theta) and its gradient for theta = [log_amp, log_scale_1..d] of the
 * Matern-3/2 ARD kernel with fixed observation noise sigma.  A session keeps the training set (Xn: n x d row-major,
 * normalised inputs; Yn: n x m row-major) and its work space on the device; the optimiser (host, SciPy BFGS as
 * the reference's jaxopt.ScipyMinimize) calls gpf_gp_nll_eval once per step: kernel matrix from the raw inputs,
 * blocked Cholesky, alpha, log det, K^-1 = L^-T L^-1 (rocBLAS dtrsm + dgemm), and one pass over the n x n entries for the
 * 1 + d gradient sums.  *info != 0: K is not positive definite at this theta (the optimiser rejects the step). */
typedef struct gpf_nll gpf_nll;
int gpf_gp_nll_open(int device, int n, int d, int m, const double* Xn, const double* Yn, double sigma, gpf_nll** out);
int gpf_gp_nll_eval(gpf_nll* s, const double* theta, double* value, double* grad, int* info);
int gpf_gp_nll_close(gpf_nll* s);

/* ---- through-gap profiles: GaPFlow/models/profiles.py ------------------------------------------------------------ */
/* field_mask bits of both entry points; output planes come in this order, only the selected ones */
enum {
    GPF_PROFILE_Z = 1,        /* z of every level (problem form; the operator echoes its input) */
    GPF_PROFILE_U = 2,        /* u(z) */
    GPF_PROFILE_V = 4,        /* v(z) */
    GPF_PROFILE_TAU = 8       /* 6 planes: viscous stress in Voigt order xx, yy, zz, yz, xz, xy */
};
enum { GPF_PROFILE_GRADIENTS = 1 };                 /* gpf_gap_profiles flags: include grad q (np.gradient stencil) */
enum { GPF_PROFILE_BOTH = 0, GPF_PROFILE_TOP = 1, GPF_PROFILE_BOTTOM = 2, GPF_PROFILE_NONE = 3 };     /* slip modes */
/* get_velocity_profiles / get_stress_profiles (models/profiles.py:33-138, 141-1323) for n cells x nz levels.  Bit b of
 * per_cell set: input b holds one value per cell ([comp][n]), else one value for all; bits 0 q, 1 hh (h, dh/dx, dh/dy),
 * 2 dqx, 3 dqy, 4 eta, 5 zeta, 6 Ls, 7 z ([nz][n], else [nz]).  hh NULL: the gap height is each cell's last z and the slopes
 * are zero (get_velocity_profiles takes h = z[-1], profiles.py:58); dqx / dqy NULL: zero gradients.  mode: GPF_PROFILE_*
 * slip mode (both: both walls slip with Ls, top / bottom: that wall only, none: no slip).  out: [plane][nz][n] for the
 * planes of field_mask.  The slip parabola of gpf_viscous_stress, evaluated at z (csrc/closures.hpp profile_coefficients). */
int gpf_gap_profiles_op(int64_t n, int nz, const double* z, const double* q, const double* hh, const double* dqx,
                        const double* dqy, const double* eta, const double* zeta, const double* Ls, int per_cell,
                        double U, double V, int mode, int field_mask, double* out);
/* The same on the handle's current state (the q that gpf_download returns), the gap planes of GPF_FIELD_TOPO (deformed h
 * on an elastic problem) and the slip length field: ghosted rows [ix0, ix1), levels z_k = h k / (nz - 1), slip at the
 * upper wall only and the closures' shear viscosity (the branch stress.py:328-345 uses), zeta = the bulk viscosity.  flags
 * GPF_PROFILE_GRADIENTS: grad q by np.gradient over the ghosted field divided by dx, dy.  host_out: [plane][nz][ix1-ix0][Ny+2].
 * Runs on the handle's stream through a device scratch of GPF_PROFILE_SCRATCH_MB MiB (default 256) with double-buffered
 * copies to the host; reads only (the state, the step count and later steps are unchanged).  Refused: shear thinning,
 * surrogate closures, x-slab handles (no reference counterpart: profiles.py is a function of arrays). */
int gpf_gap_profiles(gpf_handle* h, int nz, int ix0, int ix1, int field_mask, int flags, double* host_out);
/* Diagnostic: time of one launch of a store-only kernel on k_gap_profiles' grid and store pattern, writing nplanes planes
 * of ncell x nlev doubles (tools/profile_time.py; no reference counterpart). */
int gpf_profile_store_probe(int device, int64_t ncell, int nlev, int nplanes, int reps, double* ms_per_pass);

/* ---- checkpoint and restart (no reference counterpart: the reference has no solution restart) ---------------------- */
/* Everything the next step of this handle depends on, as one blob of host memory, so that a handle made by gpf_create from the
 * same configuration -- in another process, with another pitch, placement or kernel form (GPF_SCATTER_MB, GPF_KEEP_ROWS,
 * GPF_CHUNKS, GPF_ROWCOEF_TABLE, GPF_SMALL_GRID) -- continues the run bit for bit.  The blob holds a header (magic, format
 * version, Nx, Ny, component counts, the parts of gpf_config that decide the arithmetic, one 64-bit digest per plane), the
 * device's run state (dt, Ekin_old, the residual ring, step, simtime, sweep parity, the last step's dt), and planes in the
 * host layout [ix][iy] with ghost cells: the current q, the q before the last fused step when the handle still has it
 * (gpf_update_closures forms the corrector-stage closures from it), h, dh/dx, dh/dy as the device holds them, an elastic gap's
 * under-relaxed displacement, undeformed gap and deformation, the slip length when there is such a field, the densities a thinning slab keeps
 * beyond its halo, and the 16 derived planes when they hold the corrector-stage closures of a stage-wise step.
 *   gpf_checkpoint_size  bytes the blob of the handle's present state needs
 *   gpf_checkpoint_save  writes it (capacity >= that size; *written may be NULL).  Reads only.
 *   gpf_checkpoint_load  on a handle after gpf_pre_run.  GPF_ERR_INVALID with a message that names the first header field that
 *                        differs, for a truncated blob, and for a digest that does not match what arrived on the device -- all
 *                        found before the handle is touched, which then stays as it was.  The planes are then written and digested
 *                        again from the handle's memory (a mismatch there is GPF_ERR_HIP and the handle needs a fresh upload).
 *                        The row profile, the row-coefficient table and its seam records are rebuilt from the loaded gap; tol and
 *                        max_it stay the handle's own and `converged` follows from the loaded residual ring.
 * Slab handles save and load their own rows; a handle connected for the peer-to-peer transport refuses gpf_checkpoint_load with
 * GPF_ERR_STATE (the mailbox sequence numbers advance on all ranks together and cannot be put back on one): restart such a run
 * with the all-gather transport.  Not saved: surrogate models, elastic slabs (GPF_ERR_INVALID). */
int gpf_checkpoint_size(gpf_handle* h, size_t* bytes);
int gpf_checkpoint_save(gpf_handle* h, void* host, size_t capacity, size_t* written);
int gpf_checkpoint_load(gpf_handle* h, const void* host, size_t bytes);
/* Diagnostic: time of one pass of k_ckpt_pack over the three planes of the current q, chunked through the scratch as
 * gpf_checkpoint_save does, without the copies to the host (tools/checkpoint_time.py; yardstick: gpf_stream_probe(3, 3, ...)). */
int gpf_checkpoint_pack_probe(gpf_handle* h, int reps, double* ms_per_pass);

/* ---- the per-step series and their gpf_*_time diagnostics ------------------------------------------------------------------ */
/* A handle records up to nine series behind its committed steps: point probes, film integrals, weighted film integrals,
 * regions, line profiles, field extrema, running statistics, step changes and, with an elastic gap, the deformation series (the sections
 * below).  Each has a diagnostic gpf_<series>_time that enqueues n steps as gpf_step does (an elastic handle's: as its host
 * does, stage-wise) and reports the time on the handle's stream.  ONE RULE holds for all nine:
 *   - the call puts aside every series but the one it times, and that one too in the modes that do not record: nothing else
 *     is launched behind the steps, and what was armed is armed again, unchanged, when the call returns (also on an error);
 *   - it leaves no records of any other series for their _read calls (0 records; probes: 0 steps): it is a stepping call in
 *     which they recorded nothing.  The timed series' _read holds what the call recorded, none in a mode that does not record;
 *   - it begins a new window of armed statistics (count 0) at the step count it leaves, unless the call itself recorded into
 *     the window (gpf_stats_time, mode 1). */

/* ---- point probes (no reference counterpart: the reference's transient tests read q on the host after every step) -------- */
/* Per-step time series at up to 256 cells, recorded on the device so that gpf_step keeps advancing whole batches.  A probe is
 * a cell (ix, iy) of the ghosted index space, 0 <= ix <= Nx+1, 0 <= iy <= Ny+1 (ghost cells show the boundary conditions).
 * For every step that is executed AND committed, one record per probe is kept: rho, jx, jy of the committed state -- the q a
 * host would download after that step -- and, with_pressure != 0, p = eos_pressure(rho) of that same state, evaluated with the
 * handle's constants by the device function gpf_eos uses.  p is the pressure OF THE COMMITTED STATE, not the corrector-stage
 * pressure plane of the derived fields (GPF_FIELD_PRESSURE).  A step that did not run (converged / max_it under honor_stop)
 * leaves no record, nor does one that was rolled back as invalid: the scalar log keeps its entry for the invalid step, the
 * probe series ends one entry earlier.  Recording only reads: q and all scalars of a run are bitwise those of the same run
 * without probes, and with no probes set no launch and no kernel argument of the step kernel differs.
 *   gpf_probes_set    replaces the handle's probes.  GPF_ERR_INVALID with a message that names the offending probe for a cell
 *                     out of range, n > 256, or with_pressure on a handle whose pressure comes from a surrogate; GPF_ERR_STATE
 *                     on a slab handle (halo_lo / halo_hi != 0) and while a stage-wise step is open.
 *   gpf_probes_clear  removes them and frees the buffers.
 *   gpf_probes_read   the records of the steps the LAST gpf_step or gpf_close_step call committed (one per closed step), host
 *                     layout [step][probe][value], value order rho, jx, jy, (p): *first_step is the step count of the first
 *                     record, *n_steps how many the call left (either may be NULL); min(*n_steps, capacity_steps) records are
 *                     copied to out (NULL: none).  The next stepping call replaces them.  GPF_ERR_STATE without probes.
 * Where they are written: one launch of k_probe_record behind every launch-per-step step and behind gpf_close_step, told the
 * step count its step produces if it commits and writing only if the device's run state shows that count and a valid state;
 * inside k_small_steps after each commit.  The device buffer, log_cap (4096) x n x values doubles (at most 32 MiB), is
 * allocated by the first stepping call after gpf_probes_set and freed by gpf_probes_clear / gpf_destroy once the stream is
 * idle.  gpf_step_unfused records through its gpf_close_step; gpf_step_timed and the slab calls record nothing. */
int gpf_probes_set(gpf_handle* h, int n, const int32_t* ix, const int32_t* iy, int with_pressure);
int gpf_probes_clear(gpf_handle* h);
int gpf_probes_read(gpf_handle* h, double* out, int64_t capacity_steps, int64_t* first_step, int64_t* n_steps);
/* Diagnostic: n steps (1..4096) enqueued as gpf_step does, *ms from the first launch to the last on the handle's stream, with
 * mode 0 no recording, 1 k_probe_record behind every step (k_small_steps: recording inside), 2 an empty kernel in
 * k_probe_record's place -- the floor of one more launch per step (tools/probe_time.py).  What is put aside, left for _read
 * and restarted: the one rule of the gpf_*_time diagnostics, above. */
int gpf_probes_time(gpf_handle* h, int64_t n, int mode, double* ms);

/* ---- film integrals (no reference counterpart: the reference leaves load, friction and flow rates to post-processing) ---- */
/* Whole-film integrals of the COMMITTED state, reduced on the device so that gpf_step keeps advancing whole batches.  A record
 * is 9 + nsx + nsy doubles: the sums over the interior cells (1..Nx x 1..Ny), times dx dy, of
 *   load                      p, the equation of state's pressure of the committed density.  Dowson-Higginson is evaluated as
 *                             the reference writes it, rho / rho0 with IEEE divisions: near rho0 that stiff law turns the
 *                             last bit of rho * (1 / rho0) -- the form the probes' p and the step kernels use -- into up
 *                             to 1e-10 of p with one sign for all cells, which a sum over the film would keep.  So for
 *                             that law `load` is NOT the sum of the probes' p / GPF_FIELD_PRESSURE in every bit: it stands
 *                             about 1e-10 of itself beside it (csrc/closures.hpp film_pressure)
 *   load_x, load_y            p x, p y with the cell centres x = (ix - 1/2) dx, y = (iy - 1/2) dy (centre of pressure: load_x / load)
 *   p_hx, p_hy                p dh/dx, p dh/dy: the pressure's in-plane resultant on the profiled wall
 *   tau_xz_bot, tau_yz_bot    the lower wall's shear stress (GPF_FIELD_WALL_LOWER components 4, 3 evaluated on the state)
 *   tau_xz_top, tau_yz_top    the upper wall's (GPF_FIELD_WALL_UPPER components 4, 3)
 * then flow_x[k] = sum over iy of jx h dy on interior row ix[k], then flow_y[k] = sum over ix of jy h dx on interior column
 * iy[k] (at most 8 sections each; default: the first and last interior row / column, one where the extent is 1).  These are
 * plain area / line integrals of the named fields: no sign convention (outward normal, which wall pushes which) is applied.
 * Gap planes and slip-length field are the handle's, U, V and the viscosity (piezo-viscosity included) the closures'.
 * A record is a pure function of the state: the summation order is fixed by (Nx, Ny) alone, so the same state gives the same
 * bits whatever the batch size or stride, behind a step or from gpf_integrals_now.  Recording only reads.
 *   gpf_integrals_set    arms recording after every committed step whose new step count is a multiple of `every` (>= 1) and
 *                        starts with empty records.  ix / iy NULL (or nsx / nsy <= 0): the default sections.  GPF_ERR_INVALID
 *                        with a message that names the offending section for a row outside 1..Nx, a column outside 1..Ny or
 *                        more than 8; GPF_ERR_STATE on a slab and while a stage-wise step is open; GPF_ERR_INVALID with
 *                        surrogate closures or shear thinning.  An elastic gap is recorded behind gpf_elastic_update (see
 *                        "deformation series", below: WHEN).
 *   gpf_integrals_clear  disarms and frees the buffers.
 *   gpf_integrals_read   the records of the LAST gpf_step call, [record][9 + nsx + nsy], and the step count of each in
 *                        steps_out (either may be NULL); *n_records how many the call left, min(*n_records, capacity_records)
 *                        are copied.  A batch that stopped on the device leaves the records of the steps that ran; a step that
 *                        was rolled back as invalid leaves none.  GPF_ERR_STATE unless armed.
 *   gpf_integrals_now    the same record for the current committed state (armed or not: not armed, with the default
 *                        sections), by the same two kernels; `count`: doubles `out` holds.
 * Where they are written: k_film_partial + k_film_fold (csrc/integral_kernels.hip) behind the step's launch, told the step
 * count the step produces if it commits and writing only if the device's run state shows that count and a valid state.  On
 * grids small enough for k_small_steps the record is written INSIDE the batch, after the step's commit, by film_record_block
 * (same file): one workgroup replays the two kernels' summation order on the planes it holds and leaves the same bits in the
 * same slot, so the batch is not cut and a stride costs no launch (gpf_integrals_in_batch tells which path a handle takes).
 * gpf_close_step, gpf_step_timed and the slab calls record nothing.  The
 * record buffer ((log_cap + 1) records) and a row scratch (Nx x 18 doubles) are allocated on first use and freed by
 * gpf_integrals_clear / gpf_destroy once the stream is idle.  k_film_partial fetches two columns with one 16-byte load per
 * plane where the layout and the buffers are aligned for it (always, today) and with 8-byte loads otherwise, adding in the same
 * order.  Environment variable GPF_FILM_NARROW (any value, read when those buffers are allocated): take the 8-byte loads
 * regardless -- a test switch; the records are the same in every bit. */
int gpf_integrals_set(gpf_handle* h, int64_t every, int nsx, const int32_t* ix, int nsy, const int32_t* iy);
int gpf_integrals_clear(gpf_handle* h);
int gpf_integrals_read(gpf_handle* h, double* out, int64_t capacity_records, int64_t* steps_out, int64_t* n_records);
int gpf_integrals_now(gpf_handle* h, double* out, int64_t count);
/* *yes = 1 if this handle, as it stands, records its film integrals inside k_small_steps' batch (armed, and the handle steps
 * through the one-workgroup kernel), else 0: the two-launch path behind every recorded step.  GPF_ERR_INVALID for a NULL. */
int gpf_integrals_in_batch(gpf_handle* h, int* yes);
/* Diagnostic: n steps (1..4096) enqueued as gpf_step does, *ms from the first launch to the last on the handle's stream, with
 * mode 0 no recording, 1 recording at the armed stride (tools/integrals_time.py).  The other series: the one rule of the
 * gpf_*_time diagnostics (before the point probes). */
int gpf_integrals_time(gpf_handle* h, int64_t n, int mode, double* ms);

/* ---- weighted film integrals (no reference counterpart: per-pad loads, windows and Fourier modes are post-processing there) -- */
/* The film integrals' question asked per region: for each of K weight planes w_k (1 <= K <= 8) the sums over the interior cells
 * (1..Nx x 1..Ny) of w_k(ix, iy) f(ix, iy), times dx dy, of the COMMITTED state, for the nine integrands f, in this order:
 *   p                         the pressure `load` sums (csrc/closures.hpp film_pressure, see above)
 *   h                         the gap height: the window's volume
 *   rho_h                     rho h: the mass in the window
 *   jx_h, jy_h                the mass fluxes times the gap height
 *   tau_xz_bot, tau_yz_bot    the lower wall's shear stress, as the film integrals evaluate it
 *   tau_xz_top, tau_yz_top    the upper wall's
 * A record is [K][9] doubles.  No sign convention is applied and ghost cells never contribute.  A box of ones gives the load and
 * friction of one pad, cos / sin planes the amplitude of a Fourier mode, any smooth plane a window.  A record is a pure function
 * of the state and the planes: the summation order is k_film_partial's and k_film_fold's, fixed by (Nx, Ny) alone, and a cell
 * enters as acc += w * f with the product rounded on its own (no fused multiply-add).  So a weight of exactly 1.0 adds f's own
 * bits and one of exactly 0.0 a zero, and with a plane of ones p and the four tau_* equal load and the tau_* of gpf_integrals_*
 * in every bit.  Recording only reads.
 *   gpf_weighted_set    arms recording after every committed step whose new step count is a multiple of `every` (>= 1), with
 *                       the K planes `weights`, host layout [K][Nx+2][Ny+2] (ghosted like every field; what the ghost entries
 *                       hold is ignored: the device planes carry zeros there), and starts with empty records.  The planes are
 *                       copied.  GPF_ERR_INVALID for every < 1, K outside 1..8, a weight that is not finite (the message names
 *                       plane and cell; checked on the host before anything is uploaded), surrogate closures, shear thinning or
 *                       an elastic gap; GPF_ERR_STATE on a slab and while a stage-wise step is open.
 *   gpf_weighted_clear  disarms and frees the planes and the buffers.
 *   gpf_weighted_read   the records of the LAST gpf_step call, [record][K][9], and the step count of each in steps_out (either
 *                       may be NULL); *n_records how many the call left, min(*n_records, capacity_records) are copied.  A batch
 *                       that stopped on the device leaves the records of the steps that ran; a step that was rolled back as
 *                       invalid leaves none.  GPF_ERR_STATE unless armed.
 *   gpf_weighted_now    the same record for the current committed state, by the same two kernels; `count`: doubles `out` holds
 *                       (>= 9 K).  GPF_ERR_STATE unless armed (the weights live in the handle) and on an invalid run state.
 * Where they are written: k_wfilm_partial (grid Nx x K: one workgroup per interior row and weight) + k_wfilm_fold (one workgroup
 * per weight; csrc/weighted_kernels.hip) behind the step's launch, told the step count the step produces if it commits and
 * writing only if the device's run state shows that count and a valid state.  On grids small enough for k_small_steps the batch
 * is cut at the recorded steps -- with film integrals armed too, at the union of both series' steps -- which is bitwise the same
 * run: choose a stride there.  gpf_close_step, gpf_step_timed and the slab calls record nothing.  The planes (K planes of the
 * handle's layout), the row scratch (K x Nx x 9 doubles) and the record buffer ((log_cap + 1) records) are allocated by
 * gpf_weighted_set and freed by gpf_weighted_clear / gpf_destroy once the stream is idle.  Pairs of columns are fetched with one
 * 16-byte load per plane where the buffers, the weight planes among them, are aligned for it and with 8-byte loads otherwise;
 * GPF_FILM_NARROW (any value, read by gpf_weighted_set) asks for the 8-byte loads regardless -- a test switch; same bits. */
int gpf_weighted_set(gpf_handle* h, int64_t every, int K, const double* weights /* [K][Nx+2][Ny+2] */);
int gpf_weighted_clear(gpf_handle* h);
int gpf_weighted_read(gpf_handle* h, double* out, int64_t capacity_records, int64_t* steps_out, int64_t* n_records);
int gpf_weighted_now(gpf_handle* h, double* out, int64_t count);
/* Diagnostic: n steps (1..4096) enqueued as gpf_step does, *ms from the first launch to the last on the handle's stream, with
 * mode 0 no recording, 1 recording at the armed stride (tools/weighted_time.py).  The other series: the one rule of the
 * gpf_*_time diagnostics (before the point probes). */
int gpf_weighted_time(gpf_handle* h, int64_t n, int mode, double* ms);

/* ---- field extrema (no reference counterpart: the reference's users run np.argmax on a downloaded field) ------------------ */
/* Where the extremes of the COMMITTED state sit, found on the device so that gpf_step keeps advancing whole batches.  A record
 * is seven values, each with its cell (ix, iy) of the ghosted index space, taken over the interior cells 1..Nx x 1..Ny:
 *   0 p_max, 1 p_min       eos_pressure(rho) of the committed density, by the device function the probes' p uses: bit for bit
 *                          what a probe at that cell records
 *   2 rho_max, 3 rho_min   the density
 *   4 h_min                the gap height, plane 0 of the handle's topography as the device holds it (deformed, for an elastic gap)
 *   5 u_max, 6 v_max       |jx / rho|, |jy / rho| (IEEE division)
 * Host layout: values [record][7] doubles, cells [record][7][2] int32 (ix, iy).  Candidates are ordered by ONE comparison, a
 * total order on (value, ix, iy): the larger (smaller, for a minimum) value first, then the smaller ix, then the smaller iy.
 * So ties go to the smallest ix, then the smallest iy, the result does not depend on the shape of the reduction, and a record
 * is a pure function of the state: the same bits whatever the batch size, the stride or the kernel that wrote it.  No
 * floating-point atomics, no arrival order.  A committed state has no NaN and rho >= 0; rho = 0 makes |j / rho| inf under IEEE
 * comparison (NaN for j = 0, which is never selected): this is not special-cased.  Recording only reads: q and all scalars of
 * a run are bitwise those of the same run without extrema, and with none armed no launch and no kernel argument but a null
 * pointer differs.
 *   gpf_extrema_set    arms recording after every committed step whose new step count is a multiple of `every` and starts
 *                      with empty records.  GPF_ERR_INVALID for every < 1 and on a handle whose pressure comes from a surrogate
 *                      (surrogate wall shear alone is fine); GPF_ERR_STATE on a slab and while a stage-wise step is open.
 *   gpf_extrema_clear  disarms and frees the buffers.
 *   gpf_extrema_read   the records of the LAST stepping call (gpf_step; gpf_close_step, one closed step) and the step count of
 *                      each in steps_out (values, cells, steps_out may be NULL); *n_records how many the call left,
 *                      min(*n_records, capacity_records) are copied.  A batch that stopped on the device leaves the records of
 *                      the steps that ran; a step that was rolled back as invalid leaves none.  GPF_ERR_STATE unless armed.
 *   gpf_extrema_now    the same record for the current committed state, armed or not; GPF_ERR_STATE on an invalid run state.
 * Where they are written: k_extrema_partial (one workgroup per interior row, 4 planes read) + k_extrema_fold
 * (csrc/extrema_kernels.hip) behind every launch-per-step step and behind gpf_close_step, told the step count the step produces
 * if it commits and writing only if the device's run state shows that count and a valid state; inside k_small_steps after the
 * commit, from the field the workgroup holds -- the batch is NOT cut, every = 1 keeps the whole batch in one launch.  On an
 * elastic handle the gap deforms after the step closes: the closed step's record is written by the gpf_elastic_update that
 * follows it, with the gap the handle then holds (no gpf_elastic_update, no record).  gpf_step_timed and the slab calls record
 * nothing.  Record buffers ((log_cap + 1) records) and a row scratch are allocated on first use and freed by
 * gpf_extrema_clear / gpf_destroy once the stream is idle.  Pairs of columns are fetched with one 16-byte load per plane where
 * the buffers are aligned for it and with 8-byte loads otherwise; GPF_FILM_NARROW (read when the buffers are allocated) asks for
 * the 8-byte loads regardless -- a test switch; the records are the same in every bit. */
int gpf_extrema_set(gpf_handle* h, int64_t every);
int gpf_extrema_clear(gpf_handle* h);
int gpf_extrema_read(gpf_handle* h, double* values, int32_t* cells, int64_t capacity_records, int64_t* steps_out, int64_t* n_records);
int gpf_extrema_now(gpf_handle* h, double values[7], int32_t cells[14]);
/* Diagnostic: n steps (1..4096) enqueued as gpf_step does, *ms from the first launch to the last on the handle's stream, with
 * mode 0 no recording, 1 recording at the armed stride (tools/extrema_time.py).  The other series: the one rule of the
 * gpf_*_time diagnostics (before the point probes). */
int gpf_extrema_time(gpf_handle* h, int64_t n, int mode, double* ms);

/* ---- domain series of an x-slab run (no reference counterpart: the reference is single-process) ----------------------------- */
/* The film integrals and the field extrema of the WHOLE domain, recorded by every rank of a slab run: the records above, taken
 * over the undivided problem's interior, bit for bit what the undivided handle records for the same state.  Both series reduce a
 * row to a vector and fold the rows' vectors, and slabs are cut along rows: a rank reduces its own rows (the cell centre x
 * spelled from the GLOBAL row, so that the vector is the undivided problem's own), one all-gather of doubles carries every
 * rank's vectors, and every rank folds them in the undivided order of the global rows -- so every rank holds the same record,
 * as it holds the same dt.  No floating-point atomics, no arrival order.  (gpf_integrals_* and gpf_extrema_* keep refusing a
 * slab: they speak of the handle's own interior.)
 * The cut is gapflow_amd/slab.py: partition's (csrc/slab_rows.hpp): base, rem = divmod(nx_global, nranks), the first rem ranks own
 * base + 1 rows.  A rank's message is [max_nx][32] doubles, max_nx = base + (rem > 0): per local row the film integrals' 18 sums,
 * the seven extrema and the column of each as a double; the gathered buffer is [nranks][max_nx][32], and rows beyond a rank's own
 * count are never read.  The host owns the collective, so a record is two calls around it; with nothing set no launch and no HIP
 * call differs from a handle without the series.
 *   gpf_slab_series_set        describes the cut -- row0: global interior rows below this handle's first; the handle's Nx rows must
 *                              be one rank's slab of nx_global rows cut into nranks -- and arms the film integrals at the stride
 *                              every_integrals and the extrema at every_extrema (0: that series is off; both 0: only
 *                              gpf_slab_series_now_*).  Sections as gpf_integrals_set's, but GLOBAL: rows 1..nx_global, columns
 *                              1..Ny, NULL / 0: the first and last of the domain; the same messages.  Allocates the message and
 *                              the records ((log_cap + 1) each); collective in that every rank passes the same arguments but its
 *                              own row0.  A handle with neither halo (nranks 1) is accepted and records the undivided record.
 *                              GPF_ERR_INVALID with surrogate closures, shear thinning, an elastic gap (these step stage-wise on
 *                              slabs) or a slip-length plane; GPF_ERR_STATE while a stage-wise step is open and after
 *                              gpf_p2p_connect (the peer-to-peer batches have no host between steps).
 *   gpf_slab_series_clear      disarms and frees the buffers, once the stream is idle.
 *   gpf_slab_series_message    the message in device memory and its length in doubles (valid until _set / _clear / gpf_destroy).
 *   gpf_slab_series_begin      a stepping call begins: synchronises, *base = the step count, the records of the call before go.
 *   gpf_slab_series_local      behind the gpf_step_commit of the step that takes the count to `expect`: the partials of the series
 *                              due then (expect a multiple of the stride), k_slab_film_partial / k_slab_extrema_partial, one
 *                              workgroup per local row.  No launch when none is due.
 *   gpf_slab_series_fold       behind the all-gather of the messages (`gathered`, `count` doubles = nranks * the message's): the
 *                              folds of the same series, one workgroup each, into the slot of the step among the call's records.
 *                              Like every recorder, all four kernels write only if the device's run state shows the count
 *                              `expect` and a valid state.  A call may leave log_cap records per series: GPF_ERR_INVALID beyond.
 *   gpf_slab_series_end        synchronises and takes the records of the steps the call committed to the host; *ran = how many
 *                              steps that were.  A run that stopped on the device leaves none for the steps it skipped.
 *   gpf_slab_series_read       the records of the last begin .. end, with gpf_integrals_read's / gpf_extrema_read's layout and
 *                              rules: which 0 the film integrals (values [record][9 + nsx + nsy], cells unused), 1 the extrema
 *                              (values [record][7], cells [record][7][2], ix GLOBAL in the ghosted index space); times: the
 *                              simulated time of each record (a slab keeps no per-step log on the host).  Any pointer may be NULL.
 *   gpf_slab_series_now_local, gpf_slab_series_now_fold
 *                              the two halves of both records for the current committed state, armed or not (but set), in the
 *                              slot behind a call's; the fold synchronises and hands them out.  GPF_ERR_STATE on an invalid state. */
int gpf_slab_series_set(gpf_handle* h, int row0, int nx_global, int nranks, int64_t every_integrals, int nsx, const int32_t* ix, int nsy,
                        const int32_t* iy, int64_t every_extrema);
int gpf_slab_series_clear(gpf_handle* h);
int gpf_slab_series_message(gpf_handle* h, void** message, size_t* count);
int gpf_slab_series_begin(gpf_handle* h, int64_t* base);
int gpf_slab_series_local(gpf_handle* h, int64_t expect);
int gpf_slab_series_fold(gpf_handle* h, const void* gathered, size_t count, int64_t expect);
int gpf_slab_series_end(gpf_handle* h, int64_t* ran);
int gpf_slab_series_read(gpf_handle* h, int which, double* values, int32_t* cells, double* times, int64_t capacity_records, int64_t* steps_out,
                         int64_t* n_records);
int gpf_slab_series_now_local(gpf_handle* h);
int gpf_slab_series_now_fold(gpf_handle* h, const void* gathered, size_t count, double* integrals, int64_t integrals_count, double values[7],
                             int32_t cells[14]);

/* ---- deformation series of an elastic gap (no reference counterpart: its users download the gap after every step) ---------- */
/* What the wall gives way by under the film it carries, reduced on the device.  A record is six doubles and two cells, taken
 * over the interior cells 1..Nx x 1..Ny with d = the deformation plane the handle holds (GPF_FIELD_DEFORMATION), p = the
 * pressure the film integrals' `load` sums (csrc/closures.hpp film_pressure of the committed density) and h = the deformed gap:
 *   0 d_sum     sum of d, times dx dy: the displaced volume
 *   1 d2_sum    sum of d d, times dx dy (RMS deflection: sqrt(d2_sum / area))
 *   2 p_d       sum of p d, times dx dy (the elastic work of a linear half-space is half of it; the factor is the caller's)
 *   3 h_sum     sum of h, times dx dy: the film's volume
 *   4 d_max, 5 d_min   the largest and the smallest d, each with its cell (ix, iy) of the ghosted index space
 * Host layout: values [record][6] doubles, cells [record][2][2] int32 (d_max's ix, iy, then d_min's).  The sums are added in the
 * film integrals' order (k_film_partial's pair walk, its fold tree, k_film_fold's row loop), the products d d and p d rounded on
 * their own, and multiplied by dx dy once; the extrema are ordered by the field extrema's one comparison (value, then the
 * smaller ix, then the smaller iy).  A record is a pure function of (q, gap, deformation): no floating-point atomics, the same
 * bits whatever the stride, behind a step or from gpf_elastic_series_now.  Recording only reads.
 * WHEN: an elastic gap deforms after its step closes (gpf_elastic_update), so the record of a closed step is pending at
 * gpf_close_step and written behind the launches of the gpf_elastic_update that follows, with the state, the gap and the
 * deformation the handle then holds.  A step that did not commit leaves none, nor does one whose update is never called.  The
 * film integrals of an elastic handle (gpf_integrals_*, above) are recorded at the same moment by the same rule: there, and only
 * there, gpf_close_step + gpf_elastic_update leave a film-integral record, and gpf_integrals_in_batch is 0.
 *   gpf_elastic_series_set    arms recording after every committed step whose new step count is a multiple of `every` (>= 1,
 *                             else GPF_ERR_INVALID) and starts with empty records.  GPF_ERR_STATE on a handle without an elastic
 *                             gap ("no elastic gap"), on a slab and while a stage-wise step is open; GPF_ERR_INVALID on a handle
 *                             whose pressure comes from a surrogate.
 *   gpf_elastic_series_clear  disarms and frees the buffers.
 *   gpf_elastic_series_read   the records of the LAST gpf_close_step + gpf_elastic_update (one closed step) and the step count
 *                             of each in steps_out (values, cells, steps_out may be NULL); *n_records how many the call left,
 *                             min(*n_records, capacity_records) are copied.  GPF_ERR_STATE unless armed.
 *   gpf_elastic_series_now    the same record for the state, gap and deformation the handle holds, armed or not; GPF_ERR_STATE
 *                             on an invalid run state.
 * Where they are written: k_eldef_partial (one workgroup per interior row, 3 planes read: rho, h, d) + k_eldef_fold
 * (csrc/elastic_series_kernels.hip), guarded by the device's run state like every recording kernel.  Buffers ((log_cap + 1)
 * records and a row scratch) are allocated on first use and freed by gpf_elastic_series_clear / gpf_destroy once the stream is
 * idle.  Pairs of columns are fetched with one 16-byte load per plane where the three planes are aligned for it and with 8-byte
 * loads otherwise; GPF_FILM_NARROW (read when the buffers are allocated) asks for the 8-byte loads regardless -- a test switch;
 * the records are the same in every bit. */
int gpf_elastic_series_set(gpf_handle* h, int64_t every);
int gpf_elastic_series_clear(gpf_handle* h);
int gpf_elastic_series_read(gpf_handle* h, double* values, int32_t* cells, int64_t capacity_records, int64_t* steps_out, int64_t* n_records);
int gpf_elastic_series_now(gpf_handle* h, double values[6], int32_t cells[4]);
/* Diagnostic: n steps (1..4096) as a host takes them on an elastic handle -- gpf_open_step, two stages, gpf_close_step,
 * gpf_elastic_update per step --, *ms from the first launch to the last on the handle's stream (every such call synchronises:
 * the host's share is part of it), with mode 0 no recording, 1 recording at the armed stride (tools/elastic_series_time.py).
 * gpf_integrals_time steps an elastic handle the same way.  The other series: the one rule of the gpf_*_time diagnostics
 * (before the point probes). */
int gpf_elastic_series_time(gpf_handle* h, int64_t n, int mode, double* ms);

/* ---- shear-thinning series (no reference counterpart: its users download the stress planes after every step) --------------- */
/* What a shear-thinning film (gpf_config.thinning: Eyring, Carreau) carries and what it costs its walls, reduced on the device.
 * The other film reductions refuse such a handle ("shear thinning needs grad p"); this one evaluates grad p.  Per interior cell
 * (ix, iy) of the COMMITTED state, exactly as gpf_update_closures evaluates an interior cell of a thinning handle: p = the
 * equation of state's pressure of the density at the cell and its four neighbours (ghost cells are neighbours), dpx = (p[ix+1,iy]
 * - p[ix-1,iy]) / (2 dx), dpy = (p[ix,iy+1] - p[ix,iy-1]) / (2 dy), mu0 the Newtonian viscosity (piezo-viscosity included), rate
 * the mean wall shear rate of the Newtonian profile (models/viscosity.py shear_rate_avg of dpx, dpy, h, U, V, mu0), eta = mu0
 * times the thinning factor of rate.  A record is fourteen doubles and three cells, over the interior cells 1..Nx x 1..Ny:
 *   0 load                      sum of the pressure the film integrals' `load` sums, times dx dy (tau / load: a friction coefficient)
 *   1 tau_xz_bot, 2 tau_yz_bot, 3 tau_xz_top, 4 tau_yz_top        the wall shear stresses with eta, summed, times dx dy: what
 *                               GPF_FIELD wall-stress planes hold for the committed state (gpf_update_closures), bit for bit
 *   5 tau0_xz_bot .. 8 tau0_yz_top    the same with mu0: what the film would cost without thinning; bit for bit the film
 *                               integrals' tau_* of a handle without thinning that holds the same state
 *   9 eta_sum, 10 rate_sum      sums of eta and of rate, times dx dy (means: divided by the area)
 *   11 eta_min, 12 eta_max, 13 rate_max    each with its cell (ix, iy) of the ghosted index space
 * Host layout: values [record][14] doubles, cells [record][3][2] int32 (eta_min's ix, iy, then eta_max's, then rate_max's).  The
 * sums are added in the film integrals' order (k_film_partial's pair walk, its fold tree, k_film_fold's row loop), eta and rate
 * rounded on their own, and multiplied by dx dy once; the extrema are ordered by the field extrema's one comparison (value, then
 * the smaller ix, then the smaller iy; a NaN never wins).  A record is a pure function of (q, gap, slip length): no
 * floating-point atomics, the same bits whatever the stride, behind a step or from gpf_thinning_series_now.  Recording only reads.
 * WHEN: a thinning handle steps stage-wise; the record of a closed step is written behind gpf_close_step's launches, at the armed
 * stride, if the step commits.  Where the gap is elastic too it deforms after the step closes: the record is pending at
 * gpf_close_step and written behind the gpf_elastic_update that follows, with the gap the handle then holds (the extrema's rule).
 *   gpf_thinning_series_set    arms recording after every committed step whose new step count is a multiple of `every` (>= 1,
 *                              else GPF_ERR_INVALID) and starts with empty records.  GPF_ERR_STATE on a handle without shear
 *                              thinning ("no shear thinning"), on a slab and while a stage-wise step is open; GPF_ERR_INVALID
 *                              with any surrogate closure (the analytic pressure or wall stress is replaced).
 *   gpf_thinning_series_clear  disarms and frees the buffers.
 *   gpf_thinning_series_read   the records of the LAST gpf_close_step (and its gpf_elastic_update) and the step count of each in
 *                              steps_out (values, cells, steps_out may be NULL); *n_records how many the call left,
 *                              min(*n_records, capacity_records) are copied.  GPF_ERR_STATE unless armed.
 *   gpf_thinning_series_now    the same record for the state and gap the handle holds, armed or not; GPF_ERR_STATE on an invalid
 *                              run state.
 * Where they are written: k_thin_partial (one workgroup per interior row; 6 planes read, 7 with a slip-length field, and the
 * density of the two neighbouring rows; six equations of state per cell) + k_thin_fold (csrc/thinning_series_kernels.hip),
 * guarded by the device's run state like every recording kernel.  Buffers ((log_cap + 1) records and a row scratch) are
 * allocated on first use and freed by gpf_thinning_series_clear / gpf_destroy once the stream is idle.  Pairs of columns are
 * fetched with one 16-byte load per plane where the planes are aligned for it and with 8-byte loads otherwise; GPF_FILM_NARROW
 * (read when the buffers are allocated) asks for the 8-byte loads regardless -- a test switch; the records are the same in every
 * bit.  With nothing armed no launch and no HIP call is added to a step. */
int gpf_thinning_series_set(gpf_handle* h, int64_t every);
int gpf_thinning_series_clear(gpf_handle* h);
int gpf_thinning_series_read(gpf_handle* h, double* values, int32_t* cells, int64_t capacity_records, int64_t* steps_out, int64_t* n_records);
int gpf_thinning_series_now(gpf_handle* h, double values[14], int32_t cells[6]);
/* Diagnostic: n steps (1..4096) as a host takes them on a thinning handle -- gpf_open_step, two stages, gpf_close_step per step,
 * gpf_elastic_update where the gap is elastic --, *ms from the first launch to the last on the handle's stream (every such call
 * synchronises: the host's share is part of it), with mode 0 no recording, 1 recording at the armed stride
 * (tools/thinning_series_time.py). */
int gpf_thinning_series_time(gpf_handle* h, int64_t n, int mode, double* ms);

/* ---- step changes (no reference counterpart: its users download q after every step and subtract on the host) --------------- */
/* How far the committed step n moved each conserved field, reduced on the device.  With d = q^n - q^(n-1) per field (rho, jx,
 * jy) over the interior cells 1..Nx x 1..Ny, a record is eleven doubles and three cells:
 *   0 d2_rho, 1 d2_jx, 2 d2_jy        sum of d d, times dx dy
 *   3 q2_rho, 4 q2_jx, 5 q2_jy        sum of q^n q^n, times dx dy: the relative L2 change is sqrt(d2 / q2), its rate that over dt
 *   6 dmass                           sum of d_rho h, times dx dy; h is plane 0 of the gap the handle holds
 *   7 dmax_rho, 8 dmax_jx, 9 dmax_jy  the largest |d|, each with its cell (ix, iy) of the ghosted index space
 *   10 dt                             the step size of that step (the device's dt_last)
 * Host layout: values [record][11] doubles, cells [record][3][2] int32.  No sign convention, no normalisation; ghost cells never
 * contribute.  q^n is the current q buffer and q^(n-1) the OTHER one: a fused step reads one and writes the other, the
 * one-workgroup kernel leaves both on exit, a checkpoint carries both.  d of neighbouring states is a difference of nearly equal
 * numbers and hence (almost always) exact, which makes dmass a well-conditioned measure of one step's mass defect where the
 * difference of two masses is not.  The sums are added in the film integrals' order (pair walk, fold tree, row loop), every
 * product rounded on its own, and multiplied by dx dy once; the maxima are ordered by the field extrema's one comparison (the
 * larger value, then the smaller ix, then the smaller iy).  A record is a pure function of (q^n, q^(n-1), h, dt): no
 * floating-point atomics, the same bits whatever the batch size or the stride, behind a step or from gpf_changes_now.  Recording
 * only reads: q and all scalars of a run are bitwise those of the same run without it, and with nothing armed no launch differs.
 *   gpf_changes_set    arms recording after every committed step whose new step count is a multiple of `every` (>= 1, else
 *                      GPF_ERR_INVALID) and starts with empty records.  GPF_ERR_STATE on a slab and while a stage-wise step is
 *                      open; GPF_ERR_INVALID on handles that step stage-wise -- surrogate closures, shear thinning, an elastic gap.
 *   gpf_changes_clear  disarms and frees the buffers.
 *   gpf_changes_read   the records of the LAST gpf_step call and the step count of each in steps_out (values, cells, steps_out may
 *                      be NULL); *n_records how many the call left, min(*n_records, capacity_records) are copied.  A step that
 *                      did not run or was rolled back leaves none.  GPF_ERR_STATE unless armed.
 *   gpf_changes_now    the same record for the current state against the state before the last step, armed or not.
 *                      GPF_ERR_STATE, naming the cause, when that state is not on the device: no step committed since gpf_pre_run,
 *                      an upload, a resampled start or a checkpoint without it; gpf_update_closures has reused the buffer; the last
 *                      step was stage-wise; the step plan's timing launches used it.  GPF_ERR_STATE on an invalid run state.
 * Where they are written: k_change_partial (one workgroup per interior row, 7 planes read: 56 B per cell) + k_change_fold
 * (csrc/change_kernels.hip) behind every due step of a gpf_step batch, in stream order before the next step overwrites q^(n-1),
 * guarded by the device's run state like every recording kernel.  A handle that steps through the one-workgroup kernel has its
 * batch cut at every recorded step, as for the weighted integrals.  gpf_close_step, gpf_step_timed, ensembles and the slab calls
 * record nothing.  Buffers ((log_cap + 1) records and a row scratch) are allocated on first use and freed by gpf_changes_clear /
 * gpf_destroy once the stream is idle.  16-byte pair loads where the planes are aligned for them, 8-byte loads otherwise;
 * GPF_FILM_NARROW (read when the buffers are allocated) asks for the 8-byte loads regardless -- a test switch; same bits. */
int gpf_changes_set(gpf_handle* h, int64_t every);
int gpf_changes_clear(gpf_handle* h);
int gpf_changes_read(gpf_handle* h, double* values, int32_t* cells, int64_t capacity_records, int64_t* steps_out, int64_t* n_records);
int gpf_changes_now(gpf_handle* h, double values[11], int32_t cells[6]);
/* Diagnostic: n steps (1..4096) enqueued as gpf_step does, *ms from the first launch to the last on the handle's stream, with
 * mode 0 no recording, 1 recording at the armed stride (tools/changes_time.py).  The other series: the one rule of the
 * gpf_*_time diagnostics (before the point probes). */
int gpf_changes_time(gpf_handle* h, int64_t n, int mode, double* ms);

/* ---- running field statistics (no reference counterpart: its users download q after every step and average on the host) ---- */
/* WHERE on the film something happened over a run: per cell of the GHOSTED grid (Nx+2) x (Ny+2) -- the shape q has -- and per
 * requested field, the mean, the sum of squared deviations m2, the smallest and the largest value over the recorded steps, kept
 * in accumulator planes on the device.  Fields (bits of `field_mask`, index `field`): 0 p = eos_pressure(rho) of the committed
 * density, by the device function the probes' p uses (bit for bit a probe's p); 1 rho, 2 jx, 3 jy of the committed state.
 * Quantities (index `quantity`): 0 mean, 1 m2, 2 min, 3 max.  The variance of the recorded sample is m2 / count.
 * A record is folded in behind every committed step whose new step count is a multiple of `every`, greater than `after`, and
 * reached after arming.  The n-th record of a window does, per cell, every operation rounded on its own (Welford's update):
 *     n == 1:  mean = x;  m2 = 0;  min = x;  max = x        (the accumulators are not read)
 *     n  > 1:  d = x - mean;  mean = mean + d / n;  m2 = m2 + d * (x - mean);  min = x < min ? x : min;  max = x > max ? x : max
 * with an IEEE division by (double)n and no fused multiply-add.  The planes are therefore a pure function of the sequence of
 * recorded states -- the same bits whatever the batch size and whichever kernel stepped -- and restating the recurrences on the
 * host over downloaded states reproduces them in every bit.  These are SAMPLE statistics of the recorded steps: nothing is
 * weighted by dt; t_first and t_last tell how long the window was.  Recording only reads q.
 *   gpf_stats_set    arms, or arms again from scratch (count 0).  GPF_ERR_INVALID for every < 1, after < 0, an empty mask or bits
 *                    beyond 15, and for p on a handle whose pressure comes from a surrogate (rho, jx, jy alone are fine there;
 *                    surrogate wall shear is fine with all four); GPF_ERR_STATE on a slab and while a stage-wise step is open.
 *   gpf_stats_clear  disarms and frees the planes.
 *   gpf_stats_info   the window as the last stepping call left it: records folded in, step count and simulation time of the
 *                    first and of the last (any pointer may be NULL).  GPF_ERR_STATE unless armed.
 *   gpf_stats_read   one plane, host layout [Nx+2][Ny+2] like every field; n_doubles must be (Nx+2)(Ny+2).  GPF_ERR_INVALID for a
 *                    field that is not armed or a quantity outside 0..3; GPF_ERR_STATE unless armed and while count == 0.
 * Where they are written: k_stats_update (csrc/stats_kernels.hip), one launch behind the step's launch -- gpf_step's
 * launch-per-step path and gpf_close_step (an elastic handle needs no deferral: the gap is not read) --, told the step count
 * the step produces if it commits and the record's rank n, and touching nothing unless the device's run state shows that count
 * and a valid state: a step that did not run or was rolled back leaves the planes and the count as they were.  n is host
 * arithmetic, n = expect / every - a / every with a = max(step count at arming, after); the kernel also keeps {count,
 * first_step, t_first, last_step, t_last} on the device, and every stepping call checks that count against its own
 * (GPF_ERR_STATE if they differ).  On grids small enough for k_small_steps the batch is cut at the union of the steps that film
 * integrals, weighted integrals and statistics record, which is bitwise the same run: choose a stride there.
 * gpf_pre_run, gpf_resample and gpf_checkpoint_load begin a new window (count 0) and keep stride, `after` and fields; so do
 * the diagnostic calls that step without recording (gpf_step_timed, gpf_*_time).  Checkpoints do not carry accumulators.
 * Four planes of the handle's layout per requested field are allocated by gpf_stats_set and freed by gpf_stats_clear /
 * gpf_destroy once the stream is idle.  A record reads and writes them once (72 bytes per field and cell): several steps' worth
 * of traffic for all four fields, so a stride is the sensible setting on large grids.  Column pairs go through one 16-byte
 * access per plane where the buffers are aligned for it, single cells through 8-byte ones; GPF_FILM_NARROW (any value, read by
 * gpf_stats_set) asks for 8-byte accesses throughout -- a test switch; same bits. */
int gpf_stats_set(gpf_handle* h, int64_t every, int64_t after, int field_mask);
int gpf_stats_clear(gpf_handle* h);
int gpf_stats_info(gpf_handle* h, int64_t* count, int64_t* first_step, int64_t* last_step, double* t_first, double* t_last);
int gpf_stats_read(gpf_handle* h, int field, int quantity, double* out, size_t n_doubles);
/* Diagnostic (tools/stats_time.py): *ms from the first launch to the last on the handle's stream of, mode 0, n steps (1..4096)
 * enqueued as gpf_step does with nothing recorded; 1, the same recording at the armed stride; 2, n launches of an elementwise
 * kernel that moves one record's bytes over the same planes, and no step.  The other series, and the window (modes 0 and 2
 * begin a new one): the one rule of the gpf_*_time diagnostics (before the point probes). */
int gpf_stats_time(gpf_handle* h, int64_t n, int mode, double* ms);

/* ---- region series (no reference counterpart: its users download q and mask it on the host) -------------------------------- */
/* How much of the film is in a given state, and what that part carries: the cavitated zone (rho below a threshold), the zone that
 * bears the load, the thin-film zone (h below a clearance), the area above a pressure limit.  A region is {field, lo, hi, box}:
 * interior cell (ix, iy) of the COMMITTED state belongs to it iff lo <= f && f < hi for its value f of `field` and
 * box[0] <= ix <= box[1], box[2] <= iy <= box[3] (inclusive, 1-based interior indices: the ghosted index space's 1..Nx, 1..Ny; a
 * box of four zeros is the whole interior).  field: GPF_REGION_P, the equation of state's pressure of the committed density
 * (csrc/closures.hpp eos_pressure: the p of the probes, the extrema and the statistics, so that p >= p_max of the extrema record
 * holds that record's cell); GPF_REGION_RHO, _JX, _JY, the planes of the state; GPF_REGION_H, plane 0 of the gap as the device
 * holds it.  lo and hi are doubles with lo < hi; -inf / +inf leave a side open; the comparisons are IEEE's, so -0.0 equals 0.0 and
 * a NaN value never belongs.  Ghost cells never belong.  Up to 8 regions per handle.
 * Per region a record holds
 *   nine doubles   the weighted film integrals' sums, in their order (p h rho_h jx_h jy_h tau_xz_bot tau_yz_bot tau_xz_top
 *                  tau_yz_top), over the region's cells, times dx dy.  The summation order is k_wfilm_partial's and
 *                  k_wfilm_fold's and a cell enters as acc += w * f with w exactly 1.0 (member) or 0.0 and the product rounded
 *                  on its own: on a finite state the nine values equal, in every bit, what gpf_weighted_* returns for the 0 / 1
 *                  plane of the same predicate on the same state.  +0.0 for an empty region.
 *   five int64     cells, the exact number of member cells (area = cells dx dy), and their bounding box ix_min, ix_max, iy_min,
 *                  iy_max; (-1, -1, -1, -1) behind cells = 0.  The box is taken over the indices as they are: a zone that
 *                  wraps a periodic seam reports the full extent along that axis (1 .. Nx or 1 .. Ny).
 * so a record is [K][9] doubles and [K][5] int64.  It is a pure function of the state and the region list: integer folds, a
 * fixed summation tree, no floating-point atomics, no arrival order.  Recording only reads.
 *   gpf_regions_set     arms recording after every committed step whose new step count is a multiple of `every` (>= 1) with the
 *                       K regions (copied), and starts with empty records.  GPF_ERR_INVALID for every < 1, K outside 1..8, an
 *                       unknown field, lo >= hi or a NaN bound, a box outside the interior or empty (the message names the
 *                       region), surrogate closures, shear thinning or an elastic gap; GPF_ERR_STATE on a slab and while a
 *                       stage-wise step is open.
 *   gpf_regions_clear   disarms and frees the buffers.
 *   gpf_regions_read    the records of the LAST gpf_step call, sums [record][K][9] and ints [record][K][5], and the step count
 *                       of each in steps_out (any may be NULL); *n_records how many the call left, min(*n_records,
 *                       capacity_records) are copied.  A batch that stopped on the device leaves the records of the steps that
 *                       ran; a step that was rolled back as invalid leaves none.  GPF_ERR_STATE unless armed.
 *   gpf_regions_now     the same record for the current committed state, by the same two kernels; `count`: the regions `sums`
 *                       ([count][9]) and `ints` ([count][5]) have room for (>= K).  GPF_ERR_STATE unless armed and on an
 *                       invalid run state.
 * Where they are written: k_region_partial (grid Nx x K: one workgroup per interior row and region) + k_region_fold (one
 * workgroup per region; csrc/region_kernels.hip, the predicate in csrc/regions.hpp) behind the step's launch, told the step count
 * the step produces if it commits and writing only if the device's run state shows that count and a valid state.  On grids small
 * enough for k_small_steps the batch is cut at the recorded steps -- at the union of the steps of every armed series that cuts
 * it -- which is bitwise the same run: choose a stride there.  gpf_close_step, gpf_step_timed and the slab calls record nothing.
 * The buffers (row scratch K x Nx x (9 doubles + 3 int32), (log_cap + 1) records) are allocated by gpf_regions_set and freed by
 * gpf_regions_clear / gpf_destroy once the stream is idle.  There is no plane per region: nothing is uploaded or stored per
 * cell.  Pairs of columns are fetched with one 16-byte load per plane where the buffers are aligned for it and with 8-byte loads
 * otherwise; GPF_FILM_NARROW (any value, read by gpf_regions_set) asks for the 8-byte loads regardless -- a test switch; same
 * bits. */
#define GPF_REGION_P   0
#define GPF_REGION_RHO 1
#define GPF_REGION_H   2
#define GPF_REGION_JX  3
#define GPF_REGION_JY  4
typedef struct {
    int32_t field;             /* GPF_REGION_*                                                      */
    int32_t box[4];            /* ix0, ix1, iy0, iy1, inclusive; all zeros: the whole interior      */
    double  lo, hi;            /* lo <= f < hi                                                      */
} gpf_region;
int gpf_regions_set(gpf_handle* h, int64_t every, int K, const gpf_region* regions /* [K] */);
int gpf_regions_clear(gpf_handle* h);
int gpf_regions_read(gpf_handle* h, double* sums, int64_t* ints, int64_t capacity_records, int64_t* steps_out, int64_t* n_records);
int gpf_regions_now(gpf_handle* h, double* sums, int64_t* ints, int64_t count);
/* Diagnostic: n steps (1..4096) enqueued as gpf_step does, *ms from the first launch to the last on the handle's stream, with
 * mode 0 no recording, 1 recording at the armed stride (tools/regions_time.py).  The other series: the one rule of the
 * gpf_*_time diagnostics (before the point probes). */
int gpf_regions_time(gpf_handle* h, int64_t n, int mode, double* ms);

/* ---- line profiles (viz/plotting.py:51-60, viz/animations.py:200-242: the centre lines of the written frames) --------------- */
/* The reference's plots of a 2-D run are one-dimensional: plot_frame(dim=1) and the animations draw rho, jx, jy, p, the wall shear
 * stress of both walls and h along the centre lines [1:-1, ny // 2] and [nx // 2, 1:-1] of the ghosted frames.  These entry points
 * record such lines of the COMMITTED state on the device, so that an x-t diagram needs no frame to leave it.  A line is {along, i0,
 * i1} in 1-based interior indices: along GPF_LINE_X, a profile over the interior rows ix = 1..Nx (length Nx) at column i0 = i1, or
 * the arithmetic mean over the columns i0..i1 inclusive (1 <= i0 <= i1 <= Ny); along GPF_LINE_Y, the same with the axes exchanged
 * (length Ny, rows 1 <= i0 <= i1 <= Nx).  i0 = i1 = 0 is the reference's centre line: column (Ny + 2) / 2 (row (Nx + 2) / 2), the
 * ny // 2 of the ghosted shape.  Ghost cells are never on a line.  Up to 8 lines per handle.
 * Per point nine fields, in this order: rho, jx, jy (the planes of the state), p (csrc/closures.hpp eos_pressure of the committed
 * density: the function k_probe_record calls, the same bits), h (plane 0 of the gap as the device holds it), tau_xz_bot,
 * tau_yz_bot, tau_xz_top, tau_yz_top (lower[4], lower[3], upper[4], upper[3] of cell_fields: the terms the film integrals add).
 * Record layout: for each line in order, nine fields, each `length` doubles.
 * A single-index line holds the cells' own values.  A band adds each field in a fixed order from +0.0 and divides by (double)n
 * with a true division (csrc/lines.hpp states the order so that a loop on the host can restate it): along x one wave per row,
 * lane l adding the columns i0 + l, i0 + l + 64, ... ascending and the 64 lanes folded 32, 16, .. 1 apart; along y chunks of 32
 * consecutive rows from i0 added ascending, then the chunk sums ascending.  A record is a pure function of the state and the
 * lines: no atomics, no arrival order, and the same bits whichever kernel stepped.  Recording only reads.
 *   gpf_lines_set     arms recording after every committed step whose new step count is a multiple of `every` (>= 1) with the K
 *                     lines (copied), and starts with empty records.  `capacity`: the records the device buffer holds; 0: as
 *                     many as fit 64 MiB (GPF_LINES_MB in the environment: another number of MiB), at least 1; never more than
 *                     ceil(4096 / every), what the longest batch can leave.  GPF_ERR_INVALID for every < 1, capacity < 0, K
 *                     outside 1..8, `along` neither 0 nor 1, indices outside the interior or reversed (the message names the
 *                     line), surrogate closures, shear thinning or an elastic gap; GPF_ERR_STATE on a slab and while a
 *                     stage-wise step is open.
 *   gpf_lines_clear   disarms and frees the buffers.
 *   gpf_lines_read    the records of the LAST gpf_step call, out [record][doubles of a record], and the step count of each in
 *                     steps_out (either may be NULL); *n_records how many the call left, min(*n_records, capacity_records) are
 *                     copied.  A batch that stopped on the device leaves the records of the steps that ran; a step that was
 *                     rolled back as invalid leaves none.  GPF_ERR_STATE unless armed.
 *   gpf_lines_now     the same record for the current committed state, by the same kernels: of the armed lines (K = 0, lines
 *                     NULL), or of the K lines given, with buffers of this call's own and nothing armed or disarmed.  `count`:
 *                     the doubles `out` has room for (>= those of a record).  GPF_ERR_STATE on an invalid run state, and with
 *                     no lines given unless armed.
 * Where they are written: k_line_point, k_line_band_x, k_line_band_y_partial + k_line_band_y_fold (csrc/line_kernels.hip; only the
 * kinds the lines need are launched) behind the step's launch, told the step count the step produces if it commits and writing
 * only if the device's run state shows that count and a valid state.  The buffer is bounded, so gpf_step never puts more than
 * `capacity` records into one batch: with lines armed a batch is min(n - done, 4096, capacity * every - steps since the last
 * record); a call in several batches is bitwise the call in one.  On grids small enough for k_small_steps the batch is also cut
 * at the recorded steps, like the regions'.  gpf_close_step, gpf_step_timed and the slab calls record nothing. */
#define GPF_LINE_X 0
#define GPF_LINE_Y 1
typedef struct {
    int32_t along;             /* GPF_LINE_X / GPF_LINE_Y                                           */
    int32_t i0, i1;            /* columns (along x) / rows (along y), inclusive; both 0: the centre */
} gpf_line;
int gpf_lines_set(gpf_handle* h, int64_t every, int K, const gpf_line* lines /* [K] */, int64_t capacity);
int gpf_lines_clear(gpf_handle* h);
int gpf_lines_read(gpf_handle* h, double* out, int64_t capacity_records, int64_t* steps_out, int64_t* n_records);
int gpf_lines_now(gpf_handle* h, int K, const gpf_line* lines /* [K], or NULL */, double* out, int64_t count);
/* Diagnostic: n steps (1..4096) enqueued as gpf_step does, *ms from the first launch to the last on the handle's stream, with
 * mode 0 no recording, 1 recording at the armed stride, n no more than one batch may hold (tools/lines_time.py).  The other
 * series: the one rule of the gpf_*_time diagnostics (before the point probes). */
int gpf_lines_time(gpf_handle* h, int64_t n, int mode, double* ms);

/* ---- reduced frames (no reference counterpart: the reference's pictures of a run are drawn from the frames of sol.nc) ------- */
/* A written frame is every derived field on the whole ghosted grid in double precision, through the host.  A picture or a movie
 * needs few fields, a window, a coarser lattice and single precision: these entry points record exactly that of the COMMITTED state
 * on the device, in one read-only pass.  A frame is, for each selected field, one (mx, my) array:
 *   fields   a mask of the line profiles' nine, bit f = field f in their order and with their definitions: rho, jx, jy (the
 *            state's own bits), p (eos_pressure of the committed density, bit for bit a probe's p), h (plane 0 of the gap), tau_xz_bot,
 *            tau_yz_bot, tau_xz_top, tau_yz_top (lower[4], lower[3], upper[4], upper[3] of cell_fields).  The gap and the slip length
 *            are read only if h or a stress is selected, cell_fields is evaluated only if a stress is: a rho / jx / jy / p frame reads
 *            24 bytes per window cell.
 *   window   ix0..ix1, iy0..iy1 inclusive, 1-based interior indices (four zeros: the whole interior).  Ghost cells never enter.
 *   stride   sx, sy in 1..64: the window is cut into blocks of sx x sy cells from its corner (ix0, iy0); mx = ceil((ix1 - ix0 + 1)
 *            / sx), my likewise; the last block of an axis may be ragged.  At most 65535 output rows.
 *   reduce   GPF_FRAME_SAMPLE: the value of the block's first cell (ix0 + a sx, iy0 + b sy), no arithmetic (a -0.0 stays a -0.0).
 *            GPF_FRAME_MEAN: the arithmetic mean over the block's cells inside the window, each field on its own, in this order
 *            (csrc/frames.hpp, so that a loop on the host can restate it): per column of the block a sum from +0.0 over the rows in
 *            ascending ix; those sums added from +0.0 in ascending iy; one division by (double)(rows * cols).  mean with sx = sy = 1
 *            is stored, and reported by gpf_frames_shape's callers, as sample.
 *   dtype    GPF_FRAME_F8 doubles, GPF_FRAME_F4 the double result converted once, round to nearest even.
 * Record layout: [field in mask order][a = 0..mx-1][b = 0..my-1], values of the dtype, no padding.
 * A record is a pure function of the state and the frame: no atomics, no arrival order, the same bits for every batch length,
 * stride, capacity and kernel that stepped.  Recording only reads.
 *   gpf_frames_set    arms recording after every committed step whose new step count is a multiple of `every` (>= 1) with the frame
 *                     (copied), and starts with empty records.  `capacity`: the records the device buffer holds; 0: as many as fit
 *                     64 MiB (GPF_FRAMES_MB in the environment: another number of MiB), at least 1; never more than ceil(4096 /
 *                     every).  GPF_ERR_INVALID for every < 1, capacity < 0, a null spec, an empty mask or bits beyond the nine, a
 *                     window outside the interior or reversed, a stride outside 1..64, an unknown reduce or dtype, surrogate
 *                     closures, shear thinning or an elastic gap; GPF_ERR_STATE on a slab and while a stage-wise step is open.
 *   gpf_frames_clear  disarms and frees the buffer.
 *   gpf_frames_read   the records of the LAST gpf_step call, out [record][bytes of a record], and the step count of each in
 *                     steps_out (either may be NULL); *n_records how many the call left, min(*n_records, capacity_records) are
 *                     copied.  A batch that stopped on the device leaves the records of the steps that ran; a step that was rolled
 *                     back as invalid leaves none.  GPF_ERR_STATE unless armed.
 *   gpf_frames_now    the same record for the current committed state, by the same kernels: of the armed frame (spec NULL), or of
 *                     the frame given, with a buffer of this call's own and nothing armed or disarmed.  `bytes`: what `out` has room
 *                     for (>= a record's).  GPF_ERR_STATE on an invalid run state, and without a spec unless armed.
 *   gpf_frames_shape  mx, my and the bytes of a record of `spec` on this handle's grid (each pointer may be NULL); the checks of
 *                     gpf_frames_set on the spec, no device call.
 * Where they are written: k_frame_sample or k_frame_mean (csrc/frame_kernels.hip), one launch behind the step's, told the step count
 * the step produces if it commits and writing only if the device's run state shows that count and a valid state.  The buffer is
 * bounded, so gpf_step never puts more than `capacity` records into one batch: with frames armed a batch is at most capacity * every
 * - steps since the last record; a call in several batches is bitwise the call in one.  On grids small enough for k_small_steps the
 * batch is also cut at the recorded steps, like the lines'.  gpf_close_step, gpf_step_timed and the slab calls record nothing. */
#define GPF_FRAME_SAMPLE 0
#define GPF_FRAME_MEAN 1
#define GPF_FRAME_F8 0
#define GPF_FRAME_F4 1
typedef struct {
    int32_t fields;             /* bit f: field f of rho jx jy p h tau_xz_bot tau_yz_bot tau_xz_top tau_yz_top */
    int32_t ix0, ix1, iy0, iy1; /* the window, inclusive; four zeros: the whole interior                       */
    int32_t sx, sy;             /* the block, 1..64 each                                                       */
    int32_t reduce;             /* GPF_FRAME_SAMPLE / GPF_FRAME_MEAN                                           */
    int32_t dtype;              /* GPF_FRAME_F8 / GPF_FRAME_F4                                                 */
} gpf_frame_spec;
int gpf_frames_set(gpf_handle* h, int64_t every, const gpf_frame_spec* spec, int64_t capacity);
int gpf_frames_clear(gpf_handle* h);
int gpf_frames_read(gpf_handle* h, void* out, int64_t capacity_records, int64_t* steps_out, int64_t* n_records);
int gpf_frames_now(gpf_handle* h, const gpf_frame_spec* spec /* or NULL */, void* out, int64_t bytes);
int gpf_frames_shape(gpf_handle* h, const gpf_frame_spec* spec, int32_t* mx, int32_t* my, int64_t* record_bytes);
/* Diagnostic: n steps (1..4096) enqueued as gpf_step does, *ms from the first launch to the last on the handle's stream, with
 * mode 0 no recording, 1 recording at the armed stride, n no more than one batch may hold (tools/frames_time.py).  The other
 * series: the one rule of the gpf_*_time diagnostics (before the point probes). */
int gpf_frames_time(gpf_handle* h, int64_t n, int mode, double* ms);

/* ---- ensembles (no reference counterpart: the reference runs a parameter study as one process per problem) ---------------- */
/* Many small problems advanced by ONE launch per kernel instantiation: workgroup m of k_small_ensemble runs, on member m's own
 * buffers, the very body that k_small_steps runs for a handle alone (csrc/small_kernel.hip), so a member's field, run state
 * and per-step records are bit for bit those of a solo gpf_step of the same count.  Members differ freely in grid, gap,
 * edges, equation of state, step size and stop condition; nothing is shared between them.
 * Two tiers.  LDS: a member of at most 1200 cells, ghost cells included (150 KB at 16 doubles per cell), as above.  WORKSPACE: a
 * larger member of at most 16384 cells (up to 126 x 126 interior cells) runs k_mid_ensemble (csrc/mid_kernel.hip): the same
 * phases and per-cell arithmetic on one workgroup, its 19 planes per cell in a workspace in device memory that the ensemble
 * allocates at create and frees at destroy.  Such a member's results do not depend on who else is in the ensemble nor on how
 * its steps are split into calls; they agree with its solo gpf_step (another kernel, k_step2) to rounding, not bit for bit.
 *   gpf_ensemble_create   BORROWS the m handles: it does not own them and they must outlive the ensemble.  GPF_ERR_INVALID, with
 *                         a message that names the member and the reason, for: m < 1; a null handle; the same handle twice (two
 *                         workgroups would write the same buffers); a member that the one-workgroup kernel cannot take (grid
 *                         beyond 150 KB of LDS at 16 doubles per ghosted cell AND beyond 16384 ghosted cells, shear thinning, slab halo, surrogate set, elastic
 *                         gap, or GPF_SMALL_GRID=0 in the environment); members on different devices or streams (one launch
 *                         needs one stream); film integrals, probes or extrema armed on a member.
 *                         GPF_ERR_HIP, with nothing left allocated, if the argument buffers or the workspaces cannot be had.
 *   gpf_ensemble_create2  the same with flags: 0, or GPF_ENSEMBLE_FORCE_WORKSPACE: every member gets the workspace tier, those
 *                         that fit LDS too (a cross-check of the two tiers on one problem).  gpf_ensemble_create is flags = 0.
 *   gpf_ensemble_step     n[i] steps for member i, 0 <= n[i] <= 4096 (the log's capacity); 0 leaves the member alone: it is not
 *                         launched and nothing of it is touched.  honor_stop as in gpf_step, for all members.  The members
 *                         to advance are grouped by tier and instantiation (equation of state, slip-length field present or not);
 *                         each group is one launch on the members' stream with one workgroup per member (LDS tier: with the
 *                         dynamic LDS of its largest member).  The kernels' arguments travel in one host-to-device copy per call and every
 *                         member's final run state comes back in one.  n_executed (may be NULL): m step counts afterwards.
 *                         Afterwards every advanced handle is as gpf_step(h, n[i], honor_stop, ...) leaves it, the rollback of
 *                         an invalid step included: it may be stepped alone, queried or checkpointed.  Checked before anything is
 *                         launched, for members with n[i] > 0: the refusals of gpf_ensemble_create once more (a member armed or
 *                         changed since), GPF_ERR_INVALID; gpf_pre_run not called, GPF_ERR_STATE.  A refused call changes nothing.
 *                         A HIP error once a group has been launched (GPF_ERR_HIP) is another matter: those members have moved
 *                         on the device.  No further group is launched, the launched members' states are read back and their
 *                         handles brought up to date as after a good call (n_executed is filled), then the error is returned;
 *                         only if the device no longer answers do the handles keep their old step counts (gpf_state re-reads one).
 *   gpf_ensemble_log      the per-step records member `member` left in the LAST gpf_ensemble_step: *n_entries (may be NULL) how
 *                         many -- the steps that ran, plus the record of an invalid step that was rolled back; 0 for a member
 *                         that was not advanced -- and min(*n_entries, log_capacity) of them copied to log (NULL: none).  The
 *                         records stay in the member's own device log until its next stepping call, so a caller who wants no
 *                         history pays no copy at all, and one who does pays for the members it asks for.
 *   gpf_ensemble_destroy  frees the ensemble's argument buffers; the members stay.
 *   gpf_ensemble_limits   what a member may be, for hosts that refuse before calling (any pointer may be NULL): the LDS bytes
 *                         the one-workgroup kernel may take, the doubles it keeps per ghosted cell, the most steps per member
 *                         and call (the log's capacity).  Needs no device.
 *   gpf_ensemble_limits2  likewise for the workspace tier: the most cells, ghost cells included, and the doubles per cell of a
 *                         workspace (which is that many doubles per cell, rounded up to 256 bytes).
 *   gpf_ensemble_member_info  the tier member `member` got (GPF_ENSEMBLE_TIER_*) and the bytes of its workspace (0 in the LDS
 *                         tier); either pointer may be NULL.
 * Film-integral series of an ensemble (the record of gpf_integrals_*: nine sums, flow_x, flow_y).  They belong to the ensemble,
 * not to its members -- a member with gpf_integrals_set armed on itself is still refused -- and both kernels write them inside
 * the batch (csrc/integral_kernels.hip: film_record_block), in either tier bit for bit what gpf_integrals_now gives for the same
 * state, without cutting a launch:
 *   gpf_ensemble_integrals_set    arms recording, for every member, after each of ITS committed steps whose new count is a
 *                         multiple of `every` (>= 1), and starts with empty records.  ix / iy NULL (or nsx / nsy <= 0): per
 *                         member its first and last interior row / column (one where the extent is 1).  Explicit sections
 *                         hold for all members and must lie inside every member's interior: GPF_ERR_INVALID with a message that
 *                         names the member and the section otherwise, and for every < 1 or more than 8 sections; nothing is
 *                         changed then.  Allocates, per member, LOG_CAPACITY / every + 1 records and its arguments on the device:
 *                         the new series is built first and swapped in last, as the extrema's and the probes' are, so that a
 *                         set that fails on the device (GPF_ERR_HIP) too leaves the armed series, its stride and its records
 *                         as they were.
 *   gpf_ensemble_integrals_clear  disarms and frees them.
 *   gpf_ensemble_integrals_read   the records member `member` left in the LAST gpf_ensemble_step, [record][9 + nsx + nsy], and
 *                         the step count of each in steps_out (either may be NULL); *n_records (required) how many -- the
 *                         multiples of the stride among the steps the member committed in that call, by its own count: a
 *                         member that stopped on the device leaves those of the steps that ran, a rolled-back step none, a
 *                         member with n[i] = 0 none --, min(*n_records, capacity_records) are copied.  GPF_ERR_STATE unless
 *                         armed.
 * Field-extrema series and point probes of an ensemble (the records of gpf_extrema_* and gpf_probes_*), the same way: they belong
 * to the ensemble -- a member with gpf_extrema_set or gpf_probes_set armed on itself is still refused -- and both kernels write
 * them inside the batch, behind each commit, without cutting a launch.  k_small_ensemble records through the routines of
 * k_small_steps, so an LDS-tier member's records are in every bit those of its solo batch; k_mid_ensemble records the extrema
 * with one walk of the whole workgroup over the interior (csrc/extrema_kernels.hip: extrema_record_wide; the order on
 * (value, ix, iy) is total, so the record is gpf_extrema_now's of the same state in every bit) and the probes from its workspace
 * planes.  Recording only reads.  All three ensemble series may be armed together, each at its own stride.
 *   gpf_ensemble_extrema_set    arms recording, for every member, after each of ITS committed steps whose new count is a multiple
 *                         of `every`, and starts with empty records.  GPF_ERR_INVALID for every < 1 and, naming the member, for
 *                         one whose pressure comes from a surrogate (gpf_extrema_set's refusals); nothing is changed then.
 *                         Allocates, per member, LOG_CAPACITY / every + 1 records and its arguments on the device.
 *   gpf_ensemble_extrema_clear  disarms and frees them.
 *   gpf_ensemble_extrema_read   the records member `member` left in the LAST gpf_ensemble_step with gpf_extrema_read's layout,
 *                         values [record][7], cells [record][7][2], and the step count of each in steps_out (any may be NULL);
 *                         *n_records (required) how many, by the member's own count as for the film integrals;
 *                         min(*n_records, capacity_records) are copied.  GPF_ERR_STATE unless armed.
 *   gpf_ensemble_probes_set     replaces the ensemble's probes.  per_member == 0: the nprobe[0] cells (ix, iy pairs of the ghosted
 *                         index space) hold for every member; otherwise member i has nprobe[i] cells, all members' pairs one
 *                         behind the other in `cells`.  with_pressure as gpf_probes_set's.  GPF_ERR_INVALID with a message that
 *                         names the member for a cell outside its ghosted grid, fewer than 1 or more than 256 cells, or
 *                         with_pressure on a member whose pressure comes from a surrogate; and, with the need and the limit in
 *                         bytes, when the records of one call -- LOG_CAPACITY x cells x values doubles per member, in one device
 *                         allocation -- pass the budget: 256 MiB, or GPF_ENSEMBLE_PROBES_MB (MiB, read at every set).  A failed
 *                         set leaves the ensemble as it was.
 *   gpf_ensemble_probes_clear   removes them and frees the buffers.
 *   gpf_ensemble_probes_read    the records of the steps member `member` committed in the LAST gpf_ensemble_step, layout
 *                         [step][probe][value] as gpf_probes_read's: *first_step (may be NULL) the step count of the first,
 *                         *n_records (required) how many -- none for a rolled-back step or a member with n[i] = 0 --,
 *                         min(*n_records, capacity_records) are copied to out (NULL: none).  GPF_ERR_STATE without probes.
 * The records of the call before are dropped at the next gpf_ensemble_step; _clear and gpf_ensemble_destroy free the buffers
 * once the stream is idle. */
#define GPF_ENSEMBLE_FORCE_WORKSPACE 1
enum { GPF_ENSEMBLE_TIER_LDS = 0, GPF_ENSEMBLE_TIER_WORKSPACE = 1 };
typedef struct gpf_ensemble gpf_ensemble;
int gpf_ensemble_create(gpf_handle* const* members, int m, gpf_ensemble** out);
int gpf_ensemble_step(gpf_ensemble* e, const int64_t* n, int honor_stop, int64_t* n_executed);
int gpf_ensemble_log(gpf_ensemble* e, int member, gpf_scalars_t* log, int64_t log_capacity, int64_t* n_entries);
int gpf_ensemble_destroy(gpf_ensemble* e);
int gpf_ensemble_limits(int64_t* lds_bytes, int32_t* doubles_per_cell, int64_t* max_steps);
int gpf_ensemble_create2(gpf_handle* const* members, int m, int flags, gpf_ensemble** out);
int gpf_ensemble_limits2(int64_t* mid_max_cells, int32_t* mid_doubles_per_cell);
int gpf_ensemble_member_info(gpf_ensemble* e, int member, int32_t* tier, int64_t* workspace_bytes);
int gpf_ensemble_integrals_set(gpf_ensemble* e, int64_t every, int nsx, const int32_t* ix, int nsy, const int32_t* iy);
int gpf_ensemble_integrals_clear(gpf_ensemble* e);
int gpf_ensemble_integrals_read(gpf_ensemble* e, int member, double* out, int64_t capacity_records, int64_t* steps_out, int64_t* n_records);
int gpf_ensemble_extrema_set(gpf_ensemble* e, int64_t every);
int gpf_ensemble_extrema_clear(gpf_ensemble* e);
int gpf_ensemble_extrema_read(gpf_ensemble* e, int member, double* values, int32_t* cells, int64_t capacity_records, int64_t* steps_out, int64_t* n_records);
int gpf_ensemble_probes_set(gpf_ensemble* e, int per_member, const int32_t* nprobe, const int32_t* cells, int with_pressure);
int gpf_ensemble_probes_clear(gpf_ensemble* e);
int gpf_ensemble_probes_read(gpf_ensemble* e, int member, double* out, int64_t capacity_records, int64_t* first_step, int64_t* n_records);

/* ---- resampling a state onto another grid (no reference counterpart) ------------------------------- */
/* dst's state from src's committed state, both covering the same domain with different (Nx, Ny): bilinear interpolation, over
 * src's ghosted cells at dst's interior cell centres, of rho and the flow rates jx h, jy h (h: plane 0 of the gap src holds,
 * the deformed one of an elastic handle); dst gets jx = (jx h)_interp / h_dst with its own gap, and its ghost cells from its own
 * edge rules.  Per axis, for dst cell i = 1..N_dst: s = (i - 1/2) (d_dst / d_src) + 1/2 in ONE rounding (fma),
 * i0 = floor(s) clamped to 0..N_src, w = s - i0, value = (1 - w) f[i0] + w f[i0 + 1]; an axis of extent 1 on both sides copies
 * the single interior line.  Coarsening goes through the same rule and is not conservative.
 * src is only read: its stream is synchronised first, then the kernels run on dst's stream and the call returns when they have
 * finished.  Afterwards dst is what gpf_upload of that field into GPF_FIELD_Q leaves (run state untouched: call gpf_pre_run).
 * Refused, with dst unchanged: a null handle, dst == src, handles on different devices, Lx or Ly differing by more than 1e-12
 * relative, a direction periodic on one side only, a surrogate pressure on dst (GPF_ERR_INVALID); a slab or an open stage-wise
 * step on either side, q or gap missing on either side, a source whose run state is flagged invalid, a dst that is a member
 * of a live ensemble (GPF_ERR_STATE). */
int gpf_resample(gpf_handle* dst, const gpf_handle* src);
/* Diagnostic (tools/resample_time.py): `reps` (1..10000) launches on dst's stream, *ms per launch, of mode 0 what gpf_resample
 * enqueues, 1 a kernel with the same stores of a constant and no source reads.  Both write the buffer that does NOT hold dst's
 * state: the state and the run state stay. */
int gpf_resample_time(gpf_handle* dst, const gpf_handle* src, int mode, int reps, double* ms);

/* Diagnostic: time of one pass of an elementwise kernel that reads `nin` and writes `nout` fp64 planes of
 * `doubles_per_plane` elements (16 bytes per lane, grid-stride): what THIS device streams for the byte count of a fused
 * step.  bench.py reports it beside the step kernel's HBM figure (no reference counterpart: the reference has no device). */
int gpf_stream_probe(int device, int nin, int nout, int64_t doubles_per_plane, int reps, double* ms_per_pass);

#ifdef __cplusplus
}
#endif
#endif /* GAPFLOW_HIP_H */
