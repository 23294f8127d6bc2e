// params.cpp — the reference's constants and constructor-derived quantities,
// with the drop-in CLI overrides (--Re/--Nx/--Ny/--dt).
//
// Constants: cavity-01.cpp:309-320, channel-01.cpp:287-300,
// backwards_step-01.cpp:319-334. Derivations: cavity-01.cpp:355-363,
// channel-01.cpp:336-344, backwards_step-01.cpp:377-387; SOR factor:
// cavity-01.cpp:74-78 / channel-01.cpp:76-81 (identical for nx == ny).
// Mirrors cfd_amd/params.py (checked equal in tests/test_host_logic.py).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "internal.hpp"
#include "mg.hpp"

namespace {

double omega_2d(int nx, int ny) {
  const double pi = 3.14159265358979323846;
  const double rho_j = 0.5 * (std::cos(pi / (nx + 1)) + std::cos(pi / (ny + 1)));
  const double denom = 1.0 + std::sqrt(std::max(1e-14, 1.0 - rho_j * rho_j));
  return 2.0 / denom;
}

}  // namespace

extern "C" int cfd_params_init(int case_id, double re, int nx, int ny, double dt, cfd_params* out) {
  if (!out) {
    cfd::set_last_error("null output");
    return CFD_E_ARG;
  }
  cfd_params p;
  std::memset(&p, 0, sizeof p);
  p.case_id = case_id;
  p.check_every = 1;
  p.chunk = 0;
  // the reference's own sweep order (bit-identical output) on one device; the
  // rank path (cfd_create_rank) needs CFD_ORDER_RB
  p.ordering = CFD_ORDER_LEX;
  p.sweeps_per_launch = 0;
  switch (case_id) {
    case CFD_CAVITY:
      p.nx = p.ny = 63; p.length = 1.0; p.height = 1.0; p.re = 1000.0; p.u_ref = 1.0; p.rho = 1.0;
      p.cfl = 0.5; p.final_time = 20.0; p.tol_factor = 1e-9; p.abs_tol = 0.0; p.max_iters = 10000;
      p.print_interval = 100; p.save_interval = 100;
      break;
    case CFD_CHANNEL:
      p.nx = 93; p.ny = 31; p.length = 3.0; p.height = 1.0; p.re = 100.0; p.u_ref = 1.0; p.rho = 1.0;
      p.cfl = 0.25; p.final_time = 10.0; p.tol_factor = 1e-7; p.abs_tol = 1e-10; p.max_iters = 10000;
      p.print_interval = 100; p.save_interval = 100;
      break;
    case CFD_BACKSTEP:
      p.nx = 256; p.ny = 32; p.length = 8.0; p.height = 2.0; p.re = 100.0; p.u_ref = 1.0; p.rho = 1.0;
      p.cfl = 0.2; p.final_time = 15.0; p.tol_factor = 1e-7; p.abs_tol = 1e-10; p.max_iters = 10000;
      p.print_interval = 10; p.save_interval = 10; p.h_inlet = 1.0; p.step_x = 2.0;
      break;
    case CFD_RAYLEIGH_BENARD:
      return cfd_params_init_rb(re, 0.71, nx, ny, dt, out);
    default:
      cfd::set_last_error("unknown case_id");
      return CFD_E_ARG;
  }
  if (re > 0) p.re = re;
  if (nx > 0) p.nx = nx;
  if (ny > 0) p.ny = ny;
  else if (nx > 0 && case_id == CFD_CAVITY) p.ny = nx;
  if (p.nx < 2 || p.ny < 2) {
    cfd::set_last_error("grid must have at least 2 interior cells per direction");
    return CFD_E_ARG;
  }
  if (case_id == CFD_CAVITY) {
    p.height = p.ny * p.length / p.nx;
    p.nu = p.rho * p.u_ref * p.length / p.re;
    p.dx = p.dy = p.length / p.nx;
    const double h = p.dx;
    p.dt = p.cfl * std::min(0.25 * h * h / p.nu, h / p.u_ref);
  } else {
    p.nu = p.u_ref * (case_id == CFD_CHANNEL ? p.height : p.h_inlet) / p.re;
    p.dx = p.length / p.nx;
    p.dy = p.height / p.ny;
    const double h = std::min(p.dx, p.dy);
    p.dt = p.cfl * std::min(0.25 * h * h / p.nu, h / std::max(1e-12, p.u_ref));
  }
  if (dt > 0) p.dt = dt;
  p.omega = omega_2d(p.nx, p.ny);
  p.total_steps = (int)(p.final_time / p.dt);
  if (case_id == CFD_BACKSTEP) {
    p.step_i = (int)(p.step_x / p.dx);
    p.inlet_jmax = (int)(p.h_inlet / p.dy);
    if (p.step_i <= 0 || p.step_i >= p.nx) {
      cfd::set_last_error("Step location is outside computational domain!");
      return CFD_E_ARG;
    }
  } else {
    p.inlet_jmax = p.ny;
  }
  if (!(p.dt > 0)) {
    cfd::set_last_error("Computed time step is non-positive. Check physical parameters!");
    return CFD_E_ARG;
  }
  *out = p;
  return CFD_OK;
}

// Rayleigh-Benard (BASELINE configs[4]; no reference solver, mirrors
// cfd_amd/params.py): free-fall units, H = 1, L = nx/ny, lid at rest.
extern "C" int cfd_params_init_rb(double ra, double pr, int nx, int ny, double dt, cfd_params* out) {
  if (!out) {
    cfd::set_last_error("null output");
    return CFD_E_ARG;
  }
  cfd_params p;
  std::memset(&p, 0, sizeof p);
  p.case_id = CFD_RAYLEIGH_BENARD;
  p.check_every = 1;
  p.ordering = CFD_ORDER_RB;  // (no reference solver to reproduce; BASELINE configs[4] runs on ranks)
  p.nx = nx > 0 ? nx : 256;
  p.ny = ny > 0 ? ny : 64;
  p.ra = ra > 0 ? ra : 1e6;
  p.pr = pr > 0 ? pr : 0.71;
  if (p.nx < 2 || p.ny < 2) {
    cfd::set_last_error("grid must have at least 2 interior cells per direction");
    return CFD_E_ARG;
  }
  p.height = 1.0;
  p.length = p.nx * p.height / p.ny;
  p.re = std::sqrt(p.ra / p.pr);
  p.u_ref = 0.0;
  p.rho = 1.0;
  p.cfl = 0.5;
  p.final_time = 100.0;
  p.tol_factor = 1e-9;
  p.abs_tol = 0.0;
  p.max_iters = 10000;
  p.print_interval = 100;
  p.save_interval = 100;
  p.nu = std::sqrt(p.pr / p.ra);
  p.kappa = 1.0 / std::sqrt(p.ra * p.pr);
  p.buoyancy = 1.0;
  p.t_hot = 1.0;
  p.t_cold = 0.0;
  p.t_ref = 0.5 * (p.t_hot + p.t_cold);
  p.t_perturb = 0.01;
  p.dx = p.dy = p.length / p.nx;
  const double h = p.dx;
  p.dt = dt > 0 ? dt : p.cfl * std::min(0.25 * h * h / std::max(p.nu, p.kappa), h / 1.0);
  p.omega = omega_2d(p.nx, p.ny);
  p.total_steps = (int)(p.final_time / p.dt);
  p.inlet_jmax = p.ny;
  *out = p;
  return CFD_OK;
}

// Launch-plan defaults that do not depend on the device (include/cfd_amd.h
// cfd_tuning_default); Solver::init starts from these. Measured on MI355X
// (DESIGN.md §4): cavity boundary-column bands 80 % of the interior march (open
// cases 45 %); a 16-row band floor for the channel and for every reference-order
// (lexw) march, 24 for the red-black step and cavity marches; reference-order
// wall-tile bands 75 % of the interior band up to 2048 rows, 100 % above
// (channel 160 -> 169, cavity 1024^2 160 -> 178 GLUPS; 4096^2 best at 100:
// profiles/r4_tune); LDS tiles for the cavity only.
extern "C" int cfd_tuning_default(const cfd_params* p, int knob, int* value) {
  if (!p || !value) {
    cfd::set_last_error("null argument");
    return CFD_E_ARG;
  }
  const bool cav = p->case_id == CFD_CAVITY || p->case_id == CFD_RAYLEIGH_BENARD;
  switch (knob) {
    case CFD_TUNE_LEXW_EDGE_PCT: *value = p->ny <= 2048 ? 75 : 100; return CFD_OK;
    case CFD_TUNE_PAIR_EDGE_PCT: *value = cav ? 80 : 45; return CFD_OK;
    case CFD_TUNE_MARCH_MIN_TH: *value = (p->case_id == CFD_CHANNEL || p->ordering == CFD_ORDER_LEX) ? 16 : 24; return CFD_OK;
    case CFD_TUNE_TENT_TH: *value = 64; return CFD_OK;
    case CFD_TUNE_LEXW_RAMP_PCT:  // (the step: ramp bands at least the steady height, 134 -> 140 GLUPS at
                                  // 8192x512; the cavity 4096^2 loses 6 % with it: profiles/r5/*lex*)
      *value = p->case_id == CFD_BACKSTEP ? 100 : 0;
      return CFD_OK;
    case CFD_TUNE_TILE_ROUNDS: *value = cav ? 1 : 0; return CFD_OK;
    case CFD_TUNE_MARCH_ORDER: *value = 0; return CFD_OK;
    case CFD_TUNE_LEXW_LEFT: *value = 1; return CFD_OK;
    case CFD_TUNE_LEXW_UPDOWN: *value = 1; return CFD_OK;
    case CFD_TUNE_RESIDENT:  // (the channel 4096x512: 4.96 vs lexw 10.3, red-black 5.03 vs march 8.15 us per sweep)
      *value = (cav || p->case_id == CFD_CHANNEL) ? 1 : 0;
      return CFD_OK;
    case CFD_TUNE_PAIR_WPS:
    case CFD_TUNE_WAVE_WPS:
    case CFD_TUNE_LEXW_WAVES:
      cfd::set_last_error("this knob's default is derived from the device's occupancy at cfd_create");
      return CFD_E_STATE;
    default:
      cfd::set_last_error("unknown tuning knob");
      return CFD_E_ARG;
  }
}

// Sweeps per reference-order launch on one strip when sweeps_per_launch is 0
// (Solver::lexw_ns; strips and ranks keep 3). 4, except the cavity from
// 4096^2 cells on: 5, with the source-row ring in LDS (lexw.hpp lexw_lds).
// Measured on MI355X, cavity, cap 10000 (profiles/r7/lexw_deep/README.md):
// 4096^2 221 ms per step at 4, 204-209 at 5, 207-209 at 6 (the 6-sweep launch
// is VALU-bound: 106 us against 87 at 5); 2048^2 88-91 / 96 / 109 and 1024^2
// 58 / 61 / 70 ms - there one resident round of waves leaves bands of ~20
// rows, and the deeper pipeline's fill (4NS + 3 rows per band) costs more than
// the launches it saves.
int cfd::lexw_auto_sweeps(const cfd_params& p) {
  const bool cav = p.case_id == CFD_CAVITY || p.case_id == CFD_RAYLEIGH_BENARD;
  return (cav && (long long)p.nx * p.ny >= 4096LL * 4096LL) ? 5 : 4;
}

// ------------------------------------------------------------ multigrid --
// The plans of the multigrid pressure solve (mg.hpp). Every
// constant the kernels multiply with is formed here, in the operations the
// scheme's restatement under tests/ states.
namespace {

using namespace cfd;

// omega_c of a level whose larger size is m
double mg_omega_c(int m) {
  const double pi = 3.14159265358979323846;
  return 2.0 / (1.0 + std::sin(pi / (m + 1)));
}

// What every level holds whatever its operator; returns omega_c.
double mg_level_base(MgLevelBase& L, int nx, int ny) {
  L.nx = nx;
  L.ny = ny;
  L.pitch = ((nx + 3) + 15) / 16 * 16;  // the solver's own row pitch rule (level 0: its p and f buffers)
  L.lds_p = L.lds_f = -1;
  const int m = std::max(nx, ny);
  L.coarse_sweeps = 4 * m;
  const double omega = mg_omega_c(m);
  L.one_m_omega = 1.0 - omega;
  return omega;
}

// The end of every plan builder, n levels made: valid with at least two levels and a coarsest level of at
// most MG_COARSE_CELLS cells; then the one-launch tail. `head` opens the refusals ("grid ... has no ...
// plan (grid rule): "), `second_level_rule` says what a second level needs.
template <class Level>
bool mg_finish_plan(MgPlanOf<Level>& plan, int n, const std::string& head, const char* second_level_rule, std::string& why) {
  plan.levels = n;
  const Level& C = plan.lv[n - 1];
  if (n < 2) {
    why = head + second_level_rule;
    return false;
  }
  if ((long long)C.nx * C.ny > MG_COARSE_CELLS) {
    why = head + "its coarsest level " + std::to_string(C.nx) + " x " + std::to_string(C.ny) + " holds more than " +
          std::to_string(MG_COARSE_CELLS) + " cells";
    return false;
  }
  // the one-launch tail: from the first level (>= 1) of at most MG_COARSE_CELLS
  // cells whose p and f, with those of every coarser level, fit the LDS
  int tail = n - 1;
  for (int l = n - 1; l >= 1; --l) {
    long long need = 0;
    for (int q = l; q < n; ++q) need += 2LL * (plan.lv[q].nx + 2) * (plan.lv[q].ny + 2);
    if ((long long)plan.lv[l].nx * plan.lv[l].ny > MG_COARSE_CELLS || need > MG_LDS_DOUBLES) break;
    tail = l;
  }
  plan.tail = tail;
  int off = 0;
  for (int q = tail; q < n; ++q) {
    const int cells = (plan.lv[q].nx + 2) * (plan.lv[q].ny + 2);
    plan.lv[q].lds_p = off;
    plan.lv[q].lds_f = off + cells;
    off += 2 * cells;
  }
  return true;
}

// The levels of the two semi-coarsened schemes: level 0 is the solver's grid with hx = dx, hy = dy. With
// r = (hy / hx)^2 the next level halves x only (r > 2), y only (r < 1/2) or both; a direction can be halved
// while its size is even and at least 8 and the block allows it, and a level whose chosen direction(s)
// cannot be halved is the coarsest. Valid with 2 .. MG_MAX_LEVELS levels. `block` is the step's geometry
// (MgNoBlock for the channel): it fills its own fields of a level, may forbid a halving, and is halved along.
// Block::round_up = 1 (the channel at any size) halves odd sizes too, rounding up.
template <class Level, class Block>
bool mg_semi_plan(const cfd_params& p, MgPlanOf<Level>& plan, Block block, const std::string& head,
                  const char* second_level_rule, std::string& why) {
  int nx = p.nx, ny = p.ny, a = 0, b = 0, n = 0;
  plan = MgPlanOf<Level>{};
  for (;;) {
    if (n == MG_MAX_LEVELS) {
      why = head + "more than " + std::to_string(MG_MAX_LEVELS) + " levels";
      return false;
    }
    Level& L = plan.lv[n];
    const double omega = mg_level_base(L, nx, ny);
    L.a = a;
    L.b = b;
    const double hx = std::ldexp(p.dx, a), hy = std::ldexp(p.dy, b);
    L.cx = 1.0 / (hx * hx);
    L.cy = 1.0 / (hy * hy);
    const double d = 0.5 + std::ldexp(1.0, -(a + 1));
    L.cE = L.cx / d;
    L.g = 1.0 - 1.0 / d;
    for (int k = 0; k < 16; ++k) {
      const double cw = (k & 1) ? L.cx : 0.0, ce = (k & 2) ? L.cx : L.cE;
      const double cs = (k & 4) ? L.cy : 0.0, cn = (k & 8) ? L.cy : 0.0;
      L.rdiag[k] = 1.0 / ((cw + ce) + (cs + cn));
      L.omr[k] = omega * L.rdiag[k];
    }
    block.fill(L, omega);
    ++n;
    const double q = hy / hx, r = q * q;
    const bool can_x = (Block::round_up || nx % 2 == 0) && nx >= 8 && block.can_x();
    const bool can_y = (Block::round_up || ny % 2 == 0) && ny >= 8 && block.can_y(ny);
    L.kind = -1;
    if (r > 2.0) {
      if (can_x) L.kind = MGO_X;
    } else if (r < 0.5) {
      if (can_y) L.kind = MGO_Y;
    } else if (can_x && can_y) {
      L.kind = MGO_FULL;
    }
    if (L.kind < 0) break;
    if (L.kind != MGO_Y) nx = (nx + Block::round_up) / 2, ++a, block.halve_x();
    if (L.kind != MGO_X) ny = (ny + Block::round_up) / 2, ++b, block.halve_y();
  }
  return mg_finish_plan(plan, n, head, second_level_rule, why);
}

struct MgNoBlock {
  static constexpr int round_up = 0;
  void fill(MgoLevel&, double) const {}
  bool can_x() const { return true; }
  bool can_y(int) const { return true; }
  void halve_x() {}
  void halve_y() {}
};

// The step's block, halved with the grid: si = step_i >> a and jm = inlet_jmax >> b. x can be halved while
// si is even and at least 2; y while jm is even and at least 2 and the block is at least 2 rows high - so
// a coarse cell's children are all fluid or all solid and every level keeps the pair A = (jm+1, si+1),
// B = (jm, si).
struct MgStepBlock {
  static constexpr int round_up = 0;
  int si, jm;
  void fill(MgsLevel& L, double omega) const {
    const int nx = L.nx, ny = L.ny;
    L.si = si;
    L.jm = jm;
    L.chx = L.cx * 0.5;
    L.chy = L.cy * 0.5;
    // A = (jm+1, si+1): west through the corner (cx / 2), south fluid; B = (jm, si): north through it (cy / 2), east fluid
    const double ceA = si + 1 < nx ? L.cx : L.cE, cnA = jm + 1 < ny ? L.cy : 0.0;
    L.rdA = 1.0 / ((L.chx + ceA) + (L.cy + cnA));
    const double cwB = si > 1 ? L.cx : 0.0, ceB = si < nx ? L.cx : L.cE, csB = jm > 1 ? L.cy : 0.0;
    L.rdB = 1.0 / ((cwB + ceB) + (csB + L.chy));
    L.omrA = omega * L.rdA;
    L.omrB = omega * L.rdB;
  }
  bool can_x() const { return si % 2 == 0 && si >= 2; }
  bool can_y(int ny) const { return jm % 2 == 0 && jm >= 2 && ny - jm >= 2; }
  void halve_x() { si /= 2; }
  void halve_y() { jm /= 2; }
};

std::string mg_grid_name(const cfd_params& p) { return "grid " + std::to_string(p.nx) + " x " + std::to_string(p.ny); }

// cfd_mg_open_plan and cfd_mg_step_plan: the sizes of every level
template <class Plan>
int mg_report_levels(const cfd_params* p, bool (*make)(const cfd_params&, Plan&, std::string&), int* levels, int* level_nx,
                     int* level_ny) {
  if (!p) {
    set_last_error("null params");
    return CFD_E_ARG;
  }
  Plan plan;
  std::string why;
  if (!make(*p, plan, why)) {
    set_last_error(why);
    return CFD_E_ARG;
  }
  if (levels) *levels = plan.levels;
  for (int l = 0; l < MG_MAX_LEVELS; ++l) {
    if (level_nx) level_nx[l] = l < plan.levels ? plan.lv[l].nx : 0;
    if (level_ny) level_ny[l] = l < plan.levels ? plan.lv[l].ny : 0;
  }
  return CFD_OK;
}

}  // namespace

// The cavity's plan: level l+1 (half the cells per direction) exists while both
// sizes of level l are even and the smaller is at least 8.
bool cfd::mg_make_plan(const cfd_params& p, MgPlan& plan, std::string& why) {
  if (p.case_id != CFD_CAVITY && p.case_id != CFD_RAYLEIGH_BENARD) {
    why = "multigrid covers the cavity and Rayleigh-Benard (case rule): the channel has CFD_POISSON_MULTIGRID_OPEN, "
          "the step CFD_POISSON_MULTIGRID_STEP";
    return false;
  }
  if (p.nx < 2 || p.ny < 2 || !(p.dx > 0)) {
    why = "multigrid needs a grid of at least 2 x 2 cells and dx > 0 (grid rule)";
    return false;
  }
  int nx = p.nx, ny = p.ny, n = 0;
  plan = MgPlan{};
  for (;;) {
    MgLevel& L = plan.lv[n];
    const double omega = mg_level_base(L, nx, ny);
    L.h2 = std::ldexp(1.0, 2 * n) * (p.dx * p.dx);
    L.ih2 = 1.0 / L.h2;
    const double d = 0.5 + std::ldexp(1.0, -(n + 1));
    L.cS = 1.0 / d;
    L.g = 1.0 - L.cS;
    for (int k = 0; k < 16; ++k) {
      const double ew = k & 1, ee = (k >> 1) & 1, en = (k >> 2) & 1, cs = (k & 8) ? L.cS : 1.0;
      L.rdiag[k] = 1.0 / (((ew + ee) + en) + cs);
      L.omr[k] = omega * L.rdiag[k];
    }
    ++n;
    if (!(nx % 2 == 0 && ny % 2 == 0 && std::min(nx, ny) >= 8) || n == MG_MAX_LEVELS) break;
    nx /= 2;
    ny /= 2;
  }
  return mg_finish_plan(plan, n, mg_grid_name(p) + " has no multigrid plan (grid rule): ",
                        "a second level needs both sizes even and at least 8", why);
}

extern "C" int cfd_mg_plan(const cfd_params* p, int* levels, int* coarse_nx, int* coarse_ny) {
  if (!p) {
    cfd::set_last_error("null params");
    return CFD_E_ARG;
  }
  cfd::MgPlan plan;
  std::string why;
  if (!cfd::mg_make_plan(*p, plan, why)) {
    cfd::set_last_error(why);
    return CFD_E_ARG;
  }
  if (levels) *levels = plan.levels;
  if (coarse_nx) *coarse_nx = plan.lv[plan.levels - 1].nx;
  if (coarse_ny) *coarse_ny = plan.lv[plan.levels - 1].ny;
  return CFD_OK;
}

// The channel's plan (DESIGN.md §8 "The channel"): mg_semi_plan without a block.
bool cfd::mgo_make_plan(const cfd_params& p, MgoPlan& plan, std::string& why) {
  if (p.case_id != CFD_CHANNEL) {
    why = "open multigrid covers the channel (case rule): the cavity and Rayleigh-Benard have CFD_POISSON_MULTIGRID, "
          "the step CFD_POISSON_MULTIGRID_STEP";
    return false;
  }
  if (p.nx < 2 || p.ny < 2 || !(p.dx > 0) || !(p.dy > 0)) {
    why = "open multigrid needs a grid of at least 2 x 2 cells and dx, dy > 0 (grid rule)";
    return false;
  }
  return mg_semi_plan(p, plan, MgNoBlock{}, mg_grid_name(p) + " has no open multigrid plan (grid rule): ",
                      "the direction its spacings choose cannot be halved (a size must be even and at least 8)", why);
}

extern "C" int cfd_mg_open_plan(const cfd_params* p, int* levels, int* level_nx, int* level_ny) {
  return mg_report_levels<cfd::MgoPlan>(p, cfd::mgo_make_plan, levels, level_nx, level_ny);
}

// The step's plan: mg_semi_plan with the block halved along (MgStepBlock).
bool cfd::mgs_make_plan(const cfd_params& p, MgsPlan& plan, std::string& why) {
  if (p.case_id != CFD_BACKSTEP) {
    why = "step multigrid covers the backwards-facing step (case rule): the cavity and Rayleigh-Benard have "
          "CFD_POISSON_MULTIGRID, the channel CFD_POISSON_MULTIGRID_OPEN";
    return false;
  }
  if (p.nx < 2 || p.ny < 2 || !(p.dx > 0) || !(p.dy > 0)) {
    why = "step multigrid needs a grid of at least 2 x 2 cells and dx, dy > 0 (grid rule)";
    return false;
  }
  if (p.step_i < 2 || p.step_i >= p.nx || p.inlet_jmax < 2 || p.ny - p.inlet_jmax < 2) {
    why = "step multigrid needs step_i >= 2, inlet_jmax >= 2 and a block at least 2 cells high (geometry rule): step_i " +
          std::to_string(p.step_i) + ", inlet_jmax " + std::to_string(p.inlet_jmax) + " of " + std::to_string(p.ny) + " rows";
    return false;
  }
  return mg_semi_plan(p, plan, MgStepBlock{p.step_i, p.inlet_jmax}, mg_grid_name(p) + " has no step multigrid plan (grid rule): ",
                      "the direction its spacings choose cannot be halved (a size must be even and at least 8, the block's "
                      "edge even and at least 2)",
                      why);
}

extern "C" int cfd_mg_step_plan(const cfd_params* p, int* levels, int* level_nx, int* level_ny) {
  return mg_report_levels<cfd::MgsPlan>(p, cfd::mgs_make_plan, levels, level_nx, level_ny);
}

// The cavity's plan at any size: n_{l+1} = ceil(n_l / 2) while the smaller size is at
// least 8; a direction's constants as tests/mg_any_reference.py (Direction) forms them.
namespace {

void mga_direction(MgaDir& D, int l, int n0, int n, bool has_next) {
  const double W = std::ldexp(1.0, l), w = (double)(n0 - (long long)(n - 1) * (1LL << l));
  const bool irregular = w != W;
  D.lim = irregular ? n - 1 : n;
  D.c_lo = (2.0 * W) / (W + w);
  D.c_hi = D.c_lo * (W / w);
  const int nc = (n + 1) / 2;
  D.single = n % 2 == 1;
  D.last = 0;
  D.first = n + 1;
  D.r0 = D.r1 = 0.5;
  for (int k = 0; k < 3; ++k) D.pa[k] = 0.75, D.pb[k] = 0.25;
  if (!(has_next && (D.single || irregular))) return;
  D.last = nc;
  D.first = 2 * nc - 2;
  const double wc = (double)(n0 - (long long)(nc - 1) * (1LL << (l + 1)));
  if (!D.single) {
    D.r0 = W / (W + w);
    D.r1 = w / (W + w);
  }
  const double dist = W + 0.5 * wc;  // between the last two coarse centres
  D.pb[0] = (0.5 * W) / dist;
  D.pa[0] = 1.0 - D.pb[0];
  if (D.single) {
    D.pa[1] = 1.0, D.pb[1] = 0.0;
  } else {
    D.pb[1] = (0.5 * w) / dist;
    D.pa[1] = 1.0 - D.pb[1];
  }
  D.pa[2] = 1.0, D.pb[2] = 0.0;  // (n even: cell n lies beyond the last coarse centre)
}

}  // namespace

bool cfd::mga_make_plan(const cfd_params& p, MgaPlan& plan, std::string& why) {
  if (p.case_id != CFD_CAVITY && p.case_id != CFD_RAYLEIGH_BENARD) {
    why = "any-size multigrid covers the cavity and Rayleigh-Benard (case rule): the channel has "
          "CFD_POISSON_MULTIGRID_OPEN, the step CFD_POISSON_MULTIGRID_STEP";
    return false;
  }
  if (p.nx < 2 || p.ny < 2 || !(p.dx > 0)) {
    why = "any-size multigrid needs a grid of at least 2 x 2 cells and dx > 0 (grid rule)";
    return false;
  }
  const std::string head = mg_grid_name(p) + " has no any-size multigrid plan (grid rule): ";
  int sx[MG_MAX_LEVELS], sy[MG_MAX_LEVELS], n = 0;
  for (int nx = p.nx, ny = p.ny;; nx = (nx + 1) / 2, ny = (ny + 1) / 2) {
    if (n == MG_MAX_LEVELS) {
      why = head + "more than " + std::to_string(MG_MAX_LEVELS) + " levels";
      return false;
    }
    sx[n] = nx, sy[n] = ny, ++n;
    if (std::min(nx, ny) < 8) break;
  }
  plan = MgaPlan{};
  for (int l = 0; l < n; ++l) {
    MgaLevel& L = plan.lv[l];
    const double omega = mg_level_base(L, sx[l], sy[l]);
    L.h2 = std::ldexp(1.0, 2 * l) * (p.dx * p.dx);
    L.ih2 = 1.0 / L.h2;
    const double d = 0.5 + std::ldexp(1.0, -(l + 1));
    L.cS = 1.0 / d;
    L.g = 1.0 - L.cS;
    mga_direction(L.x, l, p.nx, sx[l], l + 1 < n);
    mga_direction(L.y, l, p.ny, sy[l], l + 1 < n);
    if (n < 2) break;  // (refused below; a level under 4 cells has no four classes)
    const double ew[4] = {0.0, 1.0, 1.0, L.x.c_hi}, ee[4] = {1.0, 1.0, L.x.c_lo, 0.0};
    const double cs[4] = {L.cS, 1.0, 1.0, L.y.c_hi}, en[4] = {1.0, 1.0, L.y.c_lo, 0.0};
    for (int k = 0; k < 16; ++k) {
      L.rdiag[k] = 1.0 / (((ew[k & 3] + ee[k & 3]) + en[k >> 2]) + cs[k >> 2]);
      L.omr[k] = omega * L.rdiag[k];
    }
  }
  return mg_finish_plan(plan, n, head, "a second level needs the smaller size at least 8", why);
}

extern "C" int cfd_mg_any_plan(const cfd_params* p, int* levels, int* level_nx, int* level_ny) {
  return mg_report_levels<cfd::MgaPlan>(p, cfd::mga_make_plan, levels, level_nx, level_ny);
}

extern "C" int cfd_mg_any_level(const cfd_params* p, int level, double* out, int cap) {
  if (!p || !out) {
    cfd::set_last_error("null argument");
    return CFD_E_ARG;
  }
  cfd::MgaPlan plan;
  std::string why;
  if (!cfd::mga_make_plan(*p, plan, why)) {
    cfd::set_last_error(why);
    return CFD_E_ARG;
  }
  if (level < 0 || level >= plan.levels || cap < CFD_MG_ANY_LEVEL_DOUBLES) {
    cfd::set_last_error("cfd_mg_any_level: no such level, or fewer than CFD_MG_ANY_LEVEL_DOUBLES doubles");
    return CFD_E_ARG;
  }
  const cfd::MgaLevel& L = plan.lv[level];
  int n = 0;
  auto put = [&](double v) { out[n++] = v; };
  put(L.nx), put(L.ny), put(L.pitch), put(L.lds_p), put(L.lds_f), put(L.coarse_sweeps), put(plan.tail);
  put(L.g), put(L.one_m_omega), put(L.h2), put(L.ih2), put(L.cS);
  for (double v : L.rdiag) put(v);
  for (double v : L.omr) put(v);
  for (const cfd::MgaDir* D : {&L.x, &L.y}) {
    put(D->lim), put(D->last), put(D->single), put(D->first), put(D->c_lo), put(D->c_hi), put(D->r0), put(D->r1);
    for (double v : D->pa) put(v);
    for (double v : D->pb) put(v);
  }
  return n == CFD_MG_ANY_LEVEL_DOUBLES ? CFD_OK : CFD_E_STATE;
}

// The channel's plan at any size: mg_semi_plan halving odd sizes too, then each level's
// directions and the coefficients that depend on them, as tests/mg_open_any_reference.py (Direction, Level)
// forms them.
namespace {

struct MgRoundUpBlock : MgNoBlock {
  static constexpr int round_up = 1;
};

// One direction of a level: mga_direction with the direction's own halving count h, the face coefficients
// times c (cx or cy), no transfer constants where the level's transfer leaves the direction alone, and
// towards the east zero (x) the weight of the cell beyond the last coarse centre.
void mgoa_direction(MgaDir& D, int h, int n0, int n, double c, bool halved, bool east) {
  mga_direction(D, h, n0, n, halved);
  const double W = std::ldexp(1.0, h), w = (double)(n0 - (long long)(n - 1) * (1LL << h));
  D.c_lo = c * D.c_lo;
  D.c_hi = D.c_lo * (W / w);
  if (!halved) D.single = 0;
  if (D.last && east) {
    const double wc = (double)(n0 - (long long)(D.last - 1) * (1LL << (h + 1)));
    D.pa[2] = (w + 1.0) / (wc + 1.0);
  }
}

}  // namespace

bool cfd::mgoa_make_plan(const cfd_params& p, MgoaPlan& plan, std::string& why) {
  if (p.case_id != CFD_CHANNEL) {
    why = "any-size open multigrid covers the channel (case rule): the cavity and Rayleigh-Benard have "
          "CFD_POISSON_MULTIGRID and CFD_POISSON_MULTIGRID_ANY, the step CFD_POISSON_MULTIGRID_STEP";
    return false;
  }
  if (p.nx < 2 || p.ny < 2 || !(p.dx > 0) || !(p.dy > 0)) {
    why = "any-size open multigrid needs a grid of at least 2 x 2 cells and dx, dy > 0 (grid rule)";
    return false;
  }
  const std::string head = mg_grid_name(p) + " has no any-size open multigrid plan (grid rule): ";
  if (!mg_semi_plan(p, plan, MgRoundUpBlock{}, head,
                    "the direction its spacings choose cannot be halved (a size must be at least 8)", why))
    return false;
  for (int l = 0; l < plan.levels; ++l) {
    const MgoaLevel& L = plan.lv[l];
    if (std::min(L.nx, L.ny) < 4) {
      why = head + "its level " + std::to_string(l) + ", " + std::to_string(L.nx) + " x " + std::to_string(L.ny) +
            ", has fewer than 4 cells in a direction";
      return false;
    }
  }
  for (int l = 0; l < plan.levels; ++l) {
    MgoaLevel& L = plan.lv[l];
    mgoa_direction(L.x, L.a, p.nx, L.nx, L.cx, L.kind == MGO_FULL || L.kind == MGO_X, true);
    mgoa_direction(L.y, L.b, p.ny, L.ny, L.cy, L.kind == MGO_FULL || L.kind == MGO_Y, false);
    const double W = std::ldexp(1.0, L.a), w = (double)(p.nx - (long long)(L.nx - 1) * (1LL << L.a));
    const double d = (w + 1.0) / (2.0 * W);  // (w = W: mg_semi_plan's 0.5 + 0.5^(a+1), cE and g)
    L.cE = (L.cx / d) * (W / w);
    L.g = 1.0 - 1.0 / d;
    const double omega = mg_omega_c(std::max(L.nx, L.ny));
    const double cw[4] = {0.0, L.cx, L.cx, L.x.c_hi}, ce[4] = {L.cx, L.cx, L.x.c_lo, L.cE};
    const double cs[4] = {0.0, L.cy, L.cy, L.y.c_hi}, cn[4] = {L.cy, L.cy, L.y.c_lo, 0.0};
    for (int k = 0; k < 16; ++k) {
      L.rdiag[k] = 1.0 / ((cw[k & 3] + ce[k & 3]) + (cs[k >> 2] + cn[k >> 2]));
      L.omr[k] = omega * L.rdiag[k];
    }
  }
  return true;
}

extern "C" int cfd_mg_open_any_plan(const cfd_params* p, int* levels, int* level_nx, int* level_ny) {
  return mg_report_levels<cfd::MgoaPlan>(p, cfd::mgoa_make_plan, levels, level_nx, level_ny);
}

extern "C" int cfd_mg_open_any_level(const cfd_params* p, int level, double* out, int cap) {
  if (!p || !out) {
    cfd::set_last_error("null argument");
    return CFD_E_ARG;
  }
  cfd::MgoaPlan plan;
  std::string why;
  if (!cfd::mgoa_make_plan(*p, plan, why)) {
    cfd::set_last_error(why);
    return CFD_E_ARG;
  }
  if (level < 0 || level >= plan.levels || cap < CFD_MG_OPEN_ANY_LEVEL_DOUBLES) {
    cfd::set_last_error("cfd_mg_open_any_level: no such level, or fewer than CFD_MG_OPEN_ANY_LEVEL_DOUBLES doubles");
    return CFD_E_ARG;
  }
  const cfd::MgoaLevel& L = plan.lv[level];
  int n = 0;
  auto put = [&](double v) { out[n++] = v; };
  put(L.nx), put(L.ny), put(L.pitch), put(L.lds_p), put(L.lds_f), put(L.coarse_sweeps), put(plan.tail);
  put(L.kind), put(L.a), put(L.b);
  put(L.cx), put(L.cy), put(L.cE), put(L.g), put(L.one_m_omega);
  for (double v : L.rdiag) put(v);
  for (double v : L.omr) put(v);
  for (const cfd::MgaDir* D : {&L.x, &L.y}) {
    put(D->lim), put(D->last), put(D->single), put(D->first), put(D->c_lo), put(D->c_hi), put(D->r0), put(D->r1);
    for (double v : D->pa) put(v);
    for (double v : D->pb) put(v);
  }
  return n == CFD_MG_OPEN_ANY_LEVEL_DOUBLES ? CFD_OK : CFD_E_STATE;
}
