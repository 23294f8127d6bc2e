/*
 * include/cfd_amd.h — C-ABI of libcfd_amd.so, the MI355X-native projection
 * solver (lid-driven cavity, channel, backwards-facing step).
 *
 * The reference has no FFI: each case is one C++ class driven by main()
 * (cavity-01.cpp:306-775, channel-01.cpp:284-770, backwards_step-01.cpp:316-1062).
 * The entry points below are that class's per-timestep methods, exported with
 * plain pointers and sizes so a host in any language can bind them. Each
 * declaration names the reference method it replaces. All functions return
 * 0 on success and a negative CFD_E_* code on failure; cfd_last_error()
 * then describes the failure. No function falls back to a CPU path: if no
 * usable gfx950 device is present, cfd_create fails.
 */
#ifndef CFD_AMD_H
#define CFD_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFD_AMD_ABI_VERSION 14

/* CFD_RAYLEIGH_BENARD (BASELINE configs[4]) has no solver in the reference
 * tree (only figures): it is the cavity's projection step with a resting lid
 * plus a Boussinesq temperature field; see DESIGN.md §5c ("parity unpinned"). */
enum cfd_case { CFD_CAVITY = 0, CFD_CHANNEL = 1, CFD_BACKSTEP = 2, CFD_RAYLEIGH_BENARD = 3 };

/* Fields, named after the reference members (cavity-01.cpp:336-344). */
enum cfd_field {
  CFD_FIELD_P = 0,    /* pressure            (ny+2) x (nx+2) */
  CFD_FIELD_SRC = 1,  /* source_term         (ny+2) x (nx+2) */
  CFD_FIELD_US = 3,   /* u_tentative         (ny+2) x (nx+1) */
  CFD_FIELD_VS = 4,   /* v_tentative         (ny+1) x (nx+2) */
  CFD_FIELD_U = 5,    /* u_corrected         (ny+2) x (nx+1) */
  CFD_FIELD_V = 6,    /* v_corrected         (ny+1) x (nx+2) */
  CFD_FIELD_UC = 7,   /* u_center            (ny+2) x (nx+2) */
  CFD_FIELD_VC = 8,   /* v_center            (ny+2) x (nx+2) */
  CFD_FIELD_T = 9     /* temperature (Rayleigh-Benard only) (ny+2) x (nx+2) */
};

enum {
  CFD_OK = 0,
  CFD_E_ARG = -1,      /* invalid argument */
  CFD_E_DEVICE = -2,   /* HIP runtime / device failure */
  CFD_E_COMM = -3,     /* RCCL failure */
  CFD_E_STATE = -4,    /* call not valid in the current state */
  CFD_E_IO = -5        /* file output failure */
};

/*
 * Solver parameters: the reference's derived constants (cavity-01.cpp:322-327,
 * channel-01.cpp:302-308, backwards_step-01.cpp:337-352). Hosts derive them
 * from the CLI with cfd_params_init(); all fields may then be overridden.
 */
typedef struct cfd_params {
  int case_id;          /* enum cfd_case */
  int nx, ny;           /* global interior cells */
  double length, height;
  double re, u_ref, rho, cfl, final_time;
  double dx, dy, nu, dt, omega;
  double tol_factor, abs_tol;
  int max_iters;        /* MAX_SOR_ITERS */
  int total_steps;
  int print_interval, save_interval;
  double h_inlet, step_x;  /* backwards step geometry */
  int step_i, inlet_jmax;  /* derived step indices (backwards_step-01.cpp:386, 493) */
  int check_every;      /* residual test every N SOR iterations (1 = reference; red-black orders:
                           the reference order tests every iteration) */
  int chunk;            /* SOR launches enqueued between host polls (0 = auto) */
  int ordering;         /* CFD_ORDER_LEX (cfd_params_init's default: the reference's own sweep order,
                           bit-identical to the reference binaries - every case at any size, on strips of
                           one device and on ranks (ABI 12): the same bits at every strip / rank count) or
                           CFD_ORDER_RB (red-black: faster where the reference's solve converges, and its
                           rank launches overlap the halo exchange with the interior rows) */
  int sweeps_per_launch; /* SOR iterations fused into one kernel launch, bit-identical for every value:
                           0 = auto: red-black with the proof-mode test 4 (the backwards step on strips or
                           ranks: 3), red-black with exact residuals 3 (cavity) / 2 (channel, step);
                           lexicographic order 4 (3 on strips; the cavity from 4096^2 cells on, one
                           strip: 5); 1, 2; 3 (red-black: cavity only, every launch 3); 4 (red-black with
                           the proof test, or the lexicographic order); 5, 6 (lexicographic cavity on one
                           strip). Ignored by the one-workgroup solves (small_solve), except 6, which is
                           refused where the one-workgroup reference-order solve would take the grid */
  /* Rayleigh-Benard (case 3), free-fall units: H = 1, U = sqrt(g beta dT H),
   * nu = sqrt(Pr/Ra), kappa = 1/sqrt(Ra Pr); hot bottom wall t_hot, cold top
   * wall t_cold, adiabatic side walls; buoyancy (T - t_ref) on v. */
  double ra, pr, kappa, buoyancy, t_hot, t_cold, t_ref;
  double t_perturb;     /* initial T = conduction profile + t_perturb*sin(pi y)cos(pi x/L) */
  /* Solve-path switches (enum cfd_switch; cfd_params_init sets CFD_AUTO). None of them changes a
   * result bit (iteration counts, residuals, fields); they choose how the same solve runs. */
  int proof_test;       /* red-black launches: proof-mode convergence test where it applies -
                           every case (AUTO / ON); OFF: the max-norm residual in every tested sweep */
  int small_solve;      /* one strip, no ranks, p fits the LDS: the whole solve in one workgroup - red-black
                           (small.hpp) or the reference's order (smlex.hip) (AUTO / ON); OFF: the
                           multi-launch solve */
  int overlap;          /* ranks with >= 48 rows: halo exchange overlapped with the interior rows
                           (AUTO / ON); OFF: exchange in front of each launch */
} cfd_params;

enum cfd_switch { CFD_AUTO = 0, CFD_ON = 1, CFD_OFF = 2 };

enum cfd_ordering { CFD_ORDER_RB = 0, CFD_ORDER_LEX = 1 };

typedef struct cfd_solver cfd_solver;

typedef struct cfd_step_info {
  int sor_iterations;   /* SolverResult.first  (cavity-01.cpp:689) */
  double residual;      /* SolverResult.second (max-norm PPE residual) */
} cfd_step_info;

typedef struct cfd_stats {
  double max_divergence;      /* logStatistics, cavity-01.cpp:757-764 */
  double avg_kinetic_energy;  /* logStatistics, cavity-01.cpp:750-766 */
} cfd_stats;

typedef struct cfd_timing {
  double poisson_ms;          /* device time inside SOR launches (HIP events) */
  long long poisson_launches; /* SOR kernel launches that did work */
  long long poisson_cell_updates; /* interior cells x active iterations (this rank) */
  double step_ms;             /* device time of whole timesteps */
  long long steps;
  long long poisson_sweeps;   /* SOR iterations executed by those launches (up to 4 per fused launch) */
  long long poisson_overlapped; /* pair launches split into interior + halo-overlapped boundary rows (ranks) */
  double poisson_steady_ms;   /* lexicographic order: device time of the launches with every cell active */
  long long poisson_steady_launches; /* (the ramps at the start / end of a solve excluded) */
  long long proof_fallbacks;  /* red-black cavity: solves whose proof-mode convergence test left an
                                 iteration open, finished with exact residuals */
  int sor_kernel;             /* enum cfd_sor_kernel: the SOR kernel family of the last solve (ABI 8) */
  long long resident_timeouts; /* resident whole-solve launches whose tiles' waits timed out (never expected:
                                  the plan checks co-residency); the exact launches took those solves (ABI 12) */
  long long seqsum_chunks;        /* reference order: chunks of SQ_CH terms the sequential sums (source mean,
                                     kinetic energy) were cut into (ABI 13) */
  long long seqsum_serial_chunks; /* of those, the chunks that ran as the plain chain of adds (the first terms
                                     from zero, binade crossings, ties); the rest were exact integer sums (ABI 13) */
  long long resident_segments;    /* resident solves: segments (a resident launch, plus the exact window after an
                                     iteration it left open) summed over the solves; one per solve when every
                                     launch ran to the solve's end (ABI 14) */
} cfd_timing;

/* Which SOR kernel family ran a solve (cfd_timing.sor_kernel); every one gives the same bits for
 * the same ordering. */
enum cfd_sor_kernel {
  CFD_SOR_NONE = 0,
  CFD_SOR_MARCH = 1,  /* red-black wave-march launches (kernels.hpp), any size, strips and ranks */
  CFD_SOR_TILE = 2,   /* red-black LDS-tile launches (tile.hpp): one strip of up to ~4 M cells */
  CFD_SOR_SMALL = 3,  /* red-black whole solve in one workgroup (small.hpp): reference-sized grids */
  CFD_SOR_LEXW = 4,   /* reference order, multi-block march (lexw.hpp) */
  CFD_SOR_LEX = 5,    /* reference order, one workgroup, global memory (poisson_lex_kernel: step geometries
                         the other reference-order kernels do not take) */
  CFD_SOR_SMLEX = 6,  /* reference order, whole solve in one workgroup, p in LDS (smlex.hip): reference-sized
                         grids (ABI 9) */
  CFD_SOR_RESIDENT = 7, /* whole solve in one persistent launch, every tile of p in registers (resident.hpp):
                          the cavity and the channel, both orders, one strip of up to ~2 M cells, no ranks
                          (ABI 11) */
  CFD_SOR_MULTIGRID = 8 /* not SOR: geometric multigrid V-cycles (mg.hip), chosen with cfd_set_poisson_method;
                           its own field - converged where the SOR solves stop at their cap (added within ABI 14) */
};

/*
 * Multigrid pressure solve. Added within ABI 14: new symbols and one new enum value
 * only - no existing struct, function or default changes, and a host built against the earlier
 * ABI 14 header runs unchanged - so CFD_AMD_ABI_VERSION stays 14.
 *
 * An opt-in mode for the cavity and Rayleigh-Benard on one strip without ranks. The default solve
 * reproduces the reference's SOR, which at large grids stops at MAX_SOR_ITERS unconverged; with
 * CFD_POISSON_MULTIGRID cfd_solve_pressure / cfd_step run V(pre, post) cycles instead (red-black
 * Gauss-Seidel smoothing, full-weighting restriction, bilinear prolongation, the coarsest level by
 * a fixed number of SOR sweeps) until the reference's max-norm residual meets the reference's
 * tolerance tol_factor * max|source|, or max_cycles. cfd_step_info.sor_iterations is then the
 * cycle count and residual that max-norm residual. max_iters, ordering, check_every and the
 * solve-path switches play no part: the field is the same for every ordering.
 *
 * Plan: level 0 is the solver's grid; level l+1 (nx/2 x ny/2) exists while both sizes of level l
 * are even and the smaller is >= 8. Valid with at least two levels and a coarsest level of at most
 * 4096 cells (it is solved in one workgroup's LDS). cfd_mg_plan and cfd_set_poisson_method return
 * CFD_E_ARG, cfd_last_error naming the rule, for the channel and the step (case rule), a grid
 * without a valid plan such as the reference's 63^2 (grid rule; CFD_POISSON_MULTIGRID_ANY below takes
 * such grids), more than one strip (strip rule) and rank solvers (rank rule).
 */
enum cfd_poisson_method {
  CFD_POISSON_SOR = 0,
  CFD_POISSON_MULTIGRID = 1,      /* the cavity and Rayleigh-Benard */
  CFD_POISSON_MULTIGRID_OPEN = 2, /* the channel (below; added within ABI 14) */
  CFD_POISSON_MULTIGRID_STEP = 3, /* the backwards-facing step (below; added within ABI 14) */
  CFD_POISSON_MULTIGRID_ANY = 4,  /* the cavity and Rayleigh-Benard at any grid size (below; added within ABI 14) */
  CFD_POISSON_MULTIGRID_OPEN_ANY = 5 /* the channel at any grid size (below; added within ABI 14) */
};
typedef struct cfd_mg_options {
  int pre_sweeps, post_sweeps, max_cycles;  /* 0 (or a NULL options pointer): 2, 2, 50 */
} cfd_mg_options;
/* CFD_POISSON_SOR switches back: the next solves give the bits of a solver that never switched. */
int cfd_set_poisson_method(cfd_solver* s, int method, const cfd_mg_options* opt);
typedef struct cfd_mg_info {
  int levels, coarse_nx, coarse_ny, coarse_sweeps;  /* the plan (0 while the mode is off) */
  long long solves, cycles, launches;                /* since cfd_create / cfd_reset_timing */
  double solve_ms;  /* device time of the multigrid solves, residual passes included (HIP events) */
  double fine_ms;   /* of that, the level-0 launches (smoothing, restriction, prolongation) */
} cfd_mg_info;
int cfd_get_mg_info(cfd_solver* s, cfd_mg_info* out);
/* The plan of a parameter block (host only, no device needed); any output pointer may be NULL. */
int cfd_mg_plan(const cfd_params* p, int* levels, int* coarse_nx, int* coarse_ny);
/*
 * CFD_POISSON_MULTIGRID_OPEN: the channel's multigrid solve (DESIGN.md §8 "The channel"), a second
 * method beside the first - same options, same cfd_get_mg_info, cfd_timing.sor_kernel reports
 * CFD_SOR_MULTIGRID, CFD_POISSON_SOR switches back. New symbols and one enum value within ABI 14.
 *
 * The channel's operator (channel-01.cpp:642-688) has dx != dy, Neumann west / south / north and a
 * Dirichlet zero in the east ghost column; its solve starts from the pressure the solver holds (no
 * zeroing) and stops at tol = max(tol_factor * (max|source| or 1), abs_tol), tested on the
 * reference's own residual over ghosts refreshed as the reference refreshes them; at least one
 * cycle runs. Levels are semi-coarsened: with r = (hy / hx)^2 of a level, r > 2 halves x only,
 * r < 1/2 halves y only, otherwise both; a direction can be halved while its size is even and >= 8,
 * and a level whose chosen direction(s) cannot be halved is the coarsest. Coarse levels keep the
 * east zero where the finest grid has it. Valid with 2 .. 16 levels and a coarsest level of at most
 * 4096 cells. Refusals (CFD_E_ARG, cfd_last_error naming the rule): the cavity, Rayleigh-Benard
 * (they have CFD_POISSON_MULTIGRID and CFD_POISSON_MULTIGRID_ANY) and the step (case rule), a grid
 * without a valid plan such as
 * the reference's 93 x 31 (grid rule), more than one strip (strip rule), rank solvers (rank rule),
 * bad options.
 *
 * cfd_mg_open_plan (host only): the number of levels and every level's size in arrays of 16
 * entries (unused entries 0); any pointer may be NULL.
 */
int cfd_mg_open_plan(const cfd_params* p, int* levels, int* level_nx, int* level_ny);
/*
 * CFD_POISSON_MULTIGRID_STEP: the backwards-facing step's multigrid solve, a third
 * method beside the other two - same options, same cfd_get_mg_info, cfd_timing.sor_kernel reports
 * CFD_SOR_MULTIGRID, CFD_POISSON_SOR switches back. New symbols and one enum value within ABI 14.
 *
 * The step's operator (backwards_step-01.cpp:872-939) is the channel's over the fluid cells only:
 * the cells of the solid block (i <= step_i and j > inlet_jmax) are no unknowns, and the block's
 * corner solid, which the reference's refresh (685-740) sets to the mean of its east and its south
 * fluid cell, is eliminated into those two cells' equations on every level. The solve starts from
 * the pressure the solver holds and stops at tol = max(tol_factor * (max|source| over the fluid
 * cells, or 1), abs_tol), tested on the reference's own residual after the reference's ghost and
 * solid refresh; at least one cycle runs. Interior solid cells of p are left as they are. Levels are
 * semi-coarsened by the channel's rule with the block halved with the grid: x can be halved while
 * nx is even and >= 8 and the block's width is even and >= 2, y while ny is even and >= 8, the
 * inlet's height is even and >= 2 and the block is at least 2 rows high. Valid with 2 .. 16 levels
 * and a coarsest level of at most 4096 cells. Refusals (CFD_E_ARG, cfd_last_error naming the rule):
 * the other cases (case rule: they have methods 1, 2 and 4), step_i < 2, inlet_jmax < 2 or a block
 * fewer than 2 cells high (geometry rule), a grid without a valid plan such as 472 x 108 (grid
 * rule), more than one strip (strip rule), rank solvers (rank rule), bad options.
 *
 * cfd_mg_step_plan (host only): as cfd_mg_open_plan.
 */
int cfd_mg_step_plan(const cfd_params* p, int* levels, int* level_nx, int* level_ny);
/*
 * CFD_POISSON_MULTIGRID_ANY: the cavity's and Rayleigh-Benard's multigrid solve at any grid size
 * (DESIGN.md §8d), a fourth method beside the other three - same options, same cfd_get_mg_info,
 * cfd_timing.sor_kernel reports CFD_SOR_MULTIGRID, CFD_POISSON_SOR switches back. New symbols and
 * one enum value within ABI 14. CFD_POISSON_MULTIGRID, its bits and its refusals are unchanged.
 *
 * The solve is CFD_POISSON_MULTIGRID's (zero start, the reference's residual and tolerance) on
 * levels halved rounding up: n_{l+1} = ceil(n_l / 2) per direction while the smaller size is >= 8.
 * Cells 1 .. n_l - 1 of level l are 2^l finest cells wide, the last one what is left up to the
 * wall (1 .. 2^l), so the walls stay where the finest grid has them; the operator is the
 * finite-volume one on that grid, the restriction the volume-weighted mean over a coarse cell's
 * children (one child where n_l is odd), the prolongation linear between coarse centres and constant
 * beyond the last. Where CFD_POISSON_MULTIGRID's plan ends on a smaller size below 8 (64^2, 512^2,
 * 96 x 64) the plan, the cycle count, the residual and p are that method's, bit for bit. Valid with
 * 2 .. 16 levels and a coarsest level of at most 4096 cells: the reference's 63^2 and 93 x 31,
 * 1000^2, 4095^2, 8200^2 all have plans. Refusals (CFD_E_ARG, cfd_last_error naming the rule): the
 * channel and the step (case rule: they have methods 2 and 3), a smaller size below 8, more than 16
 * levels or a coarsest level over 4096 cells (grid rule), more than one strip (strip rule), rank
 * solvers (rank rule), bad options.
 *
 * cfd_mg_any_plan (host only): as cfd_mg_open_plan. cfd_mg_any_level (host only) writes every
 * constant of one level of the plan as doubles, for comparison with tests/mg_any_reference.py: nx,
 * ny, pitch, lds_p, lds_f, coarse_sweeps, the plan's tail; g, 1 - omega_c, h2, ih2, cS; rdiag[16];
 * omr[16]; then per direction (x, y) lim, last, single, first, c_lo, c_hi, r0, r1, pa[3], pb[3].
 * CFD_MG_ANY_LEVEL_DOUBLES doubles in all; `cap` is the room in `out`.
 */
#define CFD_MG_ANY_LEVEL_DOUBLES 72
int cfd_mg_any_plan(const cfd_params* p, int* levels, int* level_nx, int* level_ny);
int cfd_mg_any_level(const cfd_params* p, int level, double* out, int cap);
/*
 * CFD_POISSON_MULTIGRID_OPEN_ANY: the channel's multigrid solve at any grid size, a
 * fifth method beside the other four - same options, same cfd_get_mg_info, cfd_timing.sor_kernel
 * reports CFD_SOR_MULTIGRID, CFD_POISSON_SOR switches back. New symbols and one enum value within
 * ABI 14. CFD_POISSON_MULTIGRID_OPEN, its bits and its refusals are unchanged.
 *
 * The solve is CFD_POISSON_MULTIGRID_OPEN's (warm start, the reference's ghost refresh, residual and
 * tolerance, the same semi-coarsening rule) on levels halved rounding up: a direction can be halved
 * while its size is >= 8, n_{l+1} = ceil(n_l / 2). A direction halved h times has cells of 2^h
 * finest cells and a last one of what is left up to the wall (1 .. 2^h), so the walls and the east
 * zero stay where the finest grid has them; a direction a transfer does not halve is carried over.
 * The operator is the finite-volume one on that grid; column nx sees the zero (w + 1) / 2 finest
 * spacings from its centre. The restriction is the volume-weighted mean over a coarse cell's
 * children (one child where a halved size is odd), the prolongation linear between coarse centres,
 * constant beyond a Neumann end and linear towards the zero beyond the last coarse x centre. Where
 * CFD_POISSON_MULTIGRID_OPEN's plan stops on a size below 8 (96 x 32, 256 x 32, 512 x 64,
 * 4096 x 512) the plan, the cycle count, the residual and p are that method's, bit for bit. Valid
 * with 2 .. 16 levels, a coarsest level of at most 4096 cells and at least 4 cells per direction
 * on every level: the reference's 93 x 31, 126 x 90, 1000 x 100, 4000 x 500 all have plans.
 * Refusals (CFD_E_ARG, cfd_last_error naming the rule): the cavity, Rayleigh-Benard and the step
 * (case rule: they have methods 1, 4 and 3), a grid without a valid plan such as 13 x 5 (grid rule),
 * more than one strip (strip rule), rank solvers (rank rule), bad options.
 *
 * cfd_mg_open_any_plan (host only): as cfd_mg_open_plan. cfd_mg_open_any_level (host only) writes
 * every constant of one level of the plan as doubles, for comparison with
 * tests/mg_open_any_reference.py: nx, ny, pitch, lds_p, lds_f, coarse_sweeps, the plan's tail;
 * kind, a, b; cx, cy, cE, g, 1 - omega_c; rdiag[16]; omr[16]; then per direction (x, y) lim, last,
 * single, first, c_lo, c_hi, r0, r1, pa[3], pb[3]. CFD_MG_OPEN_ANY_LEVEL_DOUBLES doubles in all;
 * `cap` is the room in `out`.
 */
#define CFD_MG_OPEN_ANY_LEVEL_DOUBLES 75
int cfd_mg_open_any_plan(const cfd_params* p, int* levels, int* level_nx, int* level_ny);
int cfd_mg_open_any_level(const cfd_params* p, int level, double* out, int cap);

/* Library / ABI info. */
int cfd_abi_version(void);
const char* cfd_last_error(void);

/* Reference constants for a case with CLI overrides (<=0 / NULL keeps the
 * reference value): the constructor initialisers of the reference classes
 * (cavity-01.cpp:355-364, channel-01.cpp:336-345, backwards_step-01.cpp:377-388). */
int cfd_params_init(int case_id, double re, int nx, int ny, double dt, cfd_params* out);

/* Rayleigh-Benard parameters (no reference counterpart; BASELINE configs[4]):
 * Ra, Pr, grid (aspect L = nx/ny, H = 1, dx = dy), dt (<= 0: CFL-derived).
 * cfd_params_init(CFD_RAYLEIGH_BENARD, ra, nx, ny, dt, out) = this with Pr 0.71. */
int cfd_params_init_rb(double ra, double pr, int nx, int ny, double dt, cfd_params* out);

/* Construct a solver: CavitySolver()/ChannelSolver()/BackwardsStepSolver()
 * (cavity-01.cpp:355, channel-01.cpp:336, backwards_step-01.cpp:377) —
 * allocateFields + setupGeometry + the initial applyBoundaryConditions of the
 * open cases. The grid is split into `n_strips` row strips on this device
 * (1 = one domain, any ny >= 2); strips exchange halo rows after every stage
 * and need ny >= 8 * n_strips. */
cfd_solver* cfd_create(const cfd_params* p, int device, int n_strips);

/* Multi-process construction: this rank owns interior rows
 * [row_begin, row_end] (1-based, inclusive) of the global grid; neighbour
 * halos travel over RCCL (see cfd_comm_*). Both orderings (ABI 12: the
 * reference's order too - halo rows before every launch, the stop rule's
 * exceedance bits OR-ed over the ranks, the sequential sums chained rank to
 * rank: bit-identical to one device). */
cfd_solver* cfd_create_rank(const cfd_params* p, int device, int row_begin, int row_end, void* comm);
int cfd_destroy(cfd_solver* s);

/* Per-timestep methods. */
int cfd_apply_bc(cfd_solver* s);                  /* applyBoundaryConditions   cavity-01.cpp:523 / channel-01.cpp:509 */
int cfd_apply_tentative_bc(cfd_solver* s);        /* applyVelocityBC(u*,v*)    channel-01.cpp:369 */
int cfd_compute_tentative(cfd_solver* s);         /* computeTentativeVelocities cavity-01.cpp:548 */
/* Rayleigh-Benard only: temperature ghost cells, buoyancy added to v* and one
 * explicit advection-diffusion update of T (fused kernel); cfd_step runs it
 * between cfd_compute_tentative and cfd_build_source. */
int cfd_advance_temperature(cfd_solver* s);
int cfd_build_source(cfd_solver* s);              /* source term (+ mean removal) cavity-01.cpp:622 / channel-01.cpp:608 */
int cfd_solve_pressure(cfd_solver* s, cfd_step_info* out); /* solverPressurePoisson cavity-01.cpp:609 */
int cfd_apply_correction(cfd_solver* s);          /* applyPressureCorrection   cavity-01.cpp:695 */
int cfd_step(cfd_solver* s, cfd_step_info* out);  /* one iteration of run()'s loop, cavity-01.cpp:387-390 */
int cfd_run_steps(cfd_solver* s, int n_steps, cfd_step_info* last); /* n loop iterations, no logging */

/* interpolateToCellCenters + logStatistics reductions (cavity-01.cpp:717, 741). */
int cfd_compute_stats(cfd_solver* s, cfd_stats* out);

/* Field transfer in the reference's array shapes (see enum cfd_field), as
 * dense row-major doubles: rows x cols with rows/cols from cfd_field_shape.
 * For a rank solver only the rank's owned rows are transferred. */
int cfd_field_shape(const cfd_solver* s, int field, int* rows, int* cols);
int cfd_get_field(cfd_solver* s, int field, double* host, size_t count);
int cfd_set_field(cfd_solver* s, int field, const double* host, size_t count);

/* VTKWriter::write_structured_grid (cavity-01.cpp:95-231; masked variant
 * backwards_step-01.cpp:102-243) and write_paraview_collection
 * (cavity-01.cpp:255-287). */
int cfd_write_vtk(cfd_solver* s, const char* filename, double time_value);
int cfd_write_pvd(const char* filename, const char* const* vtk_files, const double* times, int n);

/* Host-only VTK formatting of given cell-centre / pressure arrays, each a
 * dense (ny+2) x (nx+2) row-major array in the reference's indexing. */
int cfd_write_vtk_arrays(const cfd_params* p, const char* filename, double time_value, const double* u_center,
                         const double* v_center, const double* pressure);

/* Interior rows [first, last] (global, 1-based) this solver owns. */
int cfd_owned_rows(const cfd_solver* s, int* first, int* last);

/* Launch-planning knobs (performance only: every value gives the same bits).
 * Defaults are the values measured best on MI355X. */
enum cfd_tuning {
  CFD_TUNE_PAIR_WPS = 0,      /* waves per SIMD the fused red-black launch is planned for (1..4) */
  CFD_TUNE_WAVE_WPS = 1,      /* the same for the one-sweep launch */
  CFD_TUNE_LEXW_WAVES = 2,    /* tiles per lexicographic-order launch (>= 64) */
  CFD_TUNE_LEXW_EDGE_PCT = 3, /* wall-tile band length, % of the interior band (10..100; default 75 up to
                                 2048 rows, 100 above) */
  CFD_TUNE_PAIR_EDGE_PCT = 4, /* boundary-column band length of red-black launches, % (10..100) */
  CFD_TUNE_MARCH_MIN_TH = 5,  /* minimum rows per band of a march launch (>= 1; default 16 for the channel
                                 and for the reference order, 24 for the red-black cavity / step) */
  CFD_TUNE_TENT_TH = 6,       /* rows per band of the predictor's march (>= 4) */
  CFD_TUNE_LEXW_RAMP_PCT = 7, /* lexicographic ramp launches: band height floor, % of the steady plan's (0..100;
                                 default 0, the backwards step 100) */
  CFD_TUNE_TILE_ROUNDS = 8,   /* red-black, one strip: LDS-tile launches when the grid fits this many
                                 resident rounds of tiles (one per CU; 0: never, the march launches;
                                 default 1 for the cavity, 0 for the open cases) */
  CFD_TUNE_MARCH_ORDER = 9,   /* red-black march launches: 0 = the column tiles of a band on consecutive waves
                                 (default), 1 = the bands of a column tile (ABI 9) */
  CFD_TUNE_LEXW_LEFT = 10,    /* reference-order backwards step: 1 = the column tiles left of the step's column end
                                 at the block's bottom row and march as a channel below it (default), 0 = the
                                 per-cell masked march over every row that reaches the block (ABI 10) */
  CFD_TUNE_RESIDENT = 11,     /* the cavity and the channel, one strip, no ranks, both orders (red-black: with the
                                 proof-mode test; the reference order: sampled exceedance bits, an iteration they
                                 leave open finished by the multi-block march): 1 = the whole solve as one
                                 persistent register-resident launch where the grid fits one tile per CU and every
                                 tile can be resident at once (default: cavity 1024^2 2.2 us per sweep against the
                                 LDS tiles' 5.2), 0 = never (ABI 11) */
  CFD_TUNE_LEXW_UPDOWN = 12   /* reference order, wholly active interior tiles: 1 = every other band marches up
                                 (no residuals there; neighbouring bands read their shared halo rows at the same
                                 time), 0 = every band marches down (ABI 12) */
};
int cfd_set_tuning(cfd_solver* s, int knob, int value);
/*
 * The launch plans of the most recent pressure solve (host-side bookkeeping, read only: nothing is
 * launched or planned differently for it). Added within ABI 14: one new symbol and new structs only -
 * no existing struct, default or function changes. It is what lets a test of the knobs above show
 * that a value produced the plan shape it was chosen for (tests/test_gpu_tuning.py).
 *
 * A band plan tiles rows [lo0, hi0) + [lo1, hi1) of one strip: every interior column tile in bands
 * of th rows, the first and last column tile (masked marches) in bands of `the` rows, at most `waves`
 * tiles (one resident round) unless the plan is down to one band or th is clamped. Interior bands are
 * marched in groups of 10 rows over th + extra rows, so th + extra is a multiple of 10 unless th was
 * cut to the rows there are or clamped to max_th. A solve runs several plans (proof and exact launches,
 * a shorter last launch, a replay, one plan per strip): plan[] holds each distinct one once, in the
 * order first launched, with the number of launches that ran it.
 */
enum cfd_sor_plan_kind {
  CFD_PLAN_PAIR = 0,     /* red-black fused launch of 2 - 4 sweeps (csrc/plan.hpp multi_plan) */
  CFD_PLAN_WAVE = 1,     /* red-black one-sweep launch (plan.hpp wave_bands): no boundary class (the = th),
                            no 10-row groups (extra 0) */
  CFD_PLAN_LEXW = 2,     /* reference order: the steady plan (lexw_steady_plan); the ramp launches tile by their own
                            heights, reported in cfd_sor_plan */
  CFD_PLAN_INTERIOR = 3  /* red-black ranks with halo overlap: the interior rows of a fused launch, planned for
                            the budget less the two boundary launches' tiles (those are fixed 16-row bands and
                            not reported) */
};
#define CFD_SOR_PLAN_MAX 8
typedef struct cfd_sor_band_plan {
  int kind;             /* enum cfd_sor_plan_kind */
  int sweeps;           /* SOR iterations per launch */
  int proof;            /* red-black: 1 = launched with the proof-mode test */
  int waves;            /* the wave budget: tiles of one resident round, per strip */
  int lo0, hi0, lo1, hi1;
  int ctiles;           /* column tiles */
  int th, nb0, nb1;     /* interior column tiles: band height, bands in either row range */
  int the, nbe0, nbe1;  /* boundary column tiles */
  int nl, ncx;          /* the step's red-black proof launches: column tiles left of / across the step's
                           column that form their own class (0, 0: none) */
  int tiles;            /* tiles of the plan, every class: what the planner held against the budget */
  int extra;            /* rows a wave marches beyond its band */
  int max_th;           /* most rows one wave may march (reference order: 96, from 5 sweeps on 90; else 1 << 30) */
  int budget_bands;     /* 1: the first band count came from the budget (waves / ctiles), not from the
                           CFD_TUNE_MARCH_MIN_TH floor */
  int shortened;        /* 1: the search loop then lowered the band count until the tiles fit the budget */
  int clamped;          /* 1: th was clamped to max_th (the search stops there); 2: th was cut to the rows of
                           the longer range (a band cannot be taller) */
  int march_order;      /* red-black kinds: CFD_TUNE_MARCH_ORDER as launched */
  /* reference order, the last steady launch that ran the plan (0 before one): */
  int launch_tiles;     /* tiles launched (the step's split parts included) */
  int up_bands;         /* interior bands that march up in the plain interior column tiles (odd bands, with
                           CFD_TUNE_LEXW_UPDOWN, in sampled launches; the open cases' row-checked first and
                           last bands stay down) */
  int xn, xbn;          /* the step: crossing column tiles and the bands of them split into shorter parts */
  int left_tiles;       /* the step: interior column tiles in the left class (CFD_TUNE_LEXW_LEFT), the wall
                           tile not counted */
  long long launches;   /* launches enqueued with the plan, replays included (reference order: the steady
                           ones); those enqueued past a stop exit at entry, so this may exceed
                           cfd_timing.poisson_launches */
} cfd_sor_band_plan;
typedef struct cfd_sor_plan {
  int sor_kernel;       /* enum cfd_sor_kernel of the solve (CFD_SOR_NONE before the first) */
  int n_plans;          /* entries of plan[] in use (0 for the engines that plan no bands) */
  int plans_dropped;    /* launches whose plan found no room in plan[] (never expected) */
  cfd_sor_band_plan plan[CFD_SOR_PLAN_MAX];
  /* Reference order, the ramp launches of the solve (replays and continuations included), summed over
   * the strips. Heights: the start is ceil(touched rows / waves) (ramp_by_budget) unless
   * CFD_TUNE_LEXW_RAMP_PCT % of the steady th is larger (ramp_by_floor); rounded up to 10-row groups;
   * raised by 10 while the bands exceed the 256-entry band table (ramp_grown_bands) and while the tiles
   * exceed the budget, up to the steady th (ramp_grown_tiles); past the steady th, the steady th or what
   * 256 bands need (ramp_fallback). A launch counts under one of the first two and under each of the
   * last three that changed its height. */
  long long ramp_launches;
  int ramp_th_min, ramp_th_max;       /* band heights used (0, 0: no ramp launch) */
  int ramp_nb_max, ramp_tiles_max;    /* most bands (LexRamp::nb) and most tiles of one ramp launch */
  int ramp_up;                        /* 1: some ramp launch marched a wholly active interior tile up */
  long long ramp_by_budget, ramp_by_floor, ramp_grown_bands, ramp_grown_tiles, ramp_fallback;
} cfd_sor_plan;
int cfd_sor_plan_info(cfd_solver* s, cfd_sor_plan* out);
/* The default a solver created from these parameters starts with (host only, no
 * device needed; ABI 9). The waves-per-SIMD knobs (PAIR_WPS, WAVE_WPS,
 * LEXW_WAVES) come from the device's occupancy: CFD_E_STATE. */
int cfd_tuning_default(const cfd_params* p, int knob, int* value);

/* Timing collected with HIP events on the solver's stream. */
int cfd_get_timing(cfd_solver* s, cfd_timing* out);
int cfd_reset_timing(cfd_solver* s);
int cfd_synchronize(cfd_solver* s);

/* RCCL bootstrap for multi-process strip decomposition: rank 0 creates an id
 * (opaque bytes, CFD_COMM_ID_BYTES), every rank passes it to cfd_comm_init. */
#define CFD_COMM_ID_BYTES 128
int cfd_comm_unique_id(unsigned char* id_out);
void* cfd_comm_init(const unsigned char* id, int nranks, int rank, int device);
int cfd_comm_destroy(void* comm);
/* What the transport itself reports: for RCCL, ncclCommCount / ncclCommUserRank
 * (so a host can show that RCCL saw every rank); transport 0 = RCCL, 1 = loopback. */
int cfd_comm_info(void* comm, int* nranks, int* rank, int* transport);

/* Transport check (ABI 10): one halo exchange through the solver's own send / recv group
 * (comm.hip comm_halo_exchange, as Solver::exchange issues it) with `peer` as both neighbours, on
 * device buffers of `count` doubles holding a (rank, side, index) pattern; *mismatches = doubles
 * received that differ from the peer's pattern. peer = the caller's rank exercises RCCL's send /
 * recv to self, which a one-GPU host can run. */
int cfd_comm_exchange_check(void* comm, int peer, size_t count, long long* mismatches);

/* In-process transport with the same semantics, for ranks that share one
 * device and run in separate host threads of one process (RCCL refuses two
 * ranks on one GPU): exercises the rank code path without RCCL. */
void* cfd_comm_loopback_hub(int nranks);
void* cfd_comm_init_loopback(void* hub, int rank, int device);
int cfd_comm_loopback_hub_destroy(void* hub);

#ifdef __cplusplus
}
#endif
#endif
