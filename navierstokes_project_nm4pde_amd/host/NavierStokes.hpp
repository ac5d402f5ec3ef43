// NavierStokes.hpp — C++ host mirror of the reference's `NavierStokes` class on top of the C-ABI (include/nsx.h)
// and the repository's own front-end (include/nsx_host.h).
//
// Same member names, argument meaning, call order and console output as the reference
//   Navier-Stokes/include/NavierStokes3D.hpp:10-252, NavierStokes2D.hpp, Convergence3D.hpp
//   Navier-Stokes/src/NavierStokes3D.cpp (setup :2-157, assemble :163-356, assemble_time_step :361-544,
//   solve_time_step :546-640, solve :687-741), NavierStokes2D.cpp, Convergence3D.cpp
// but every loop of the hot path runs in libnsx on the GPU.  Errors surface as C++ exceptions, as in the reference
// (SolverControl::NoConvergence -> nsx::NoConvergence, std::runtime_error for everything else).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/nsx.h"
#include "../../include/nsx_host.h"

namespace nsx {

struct NoConvergence : std::runtime_error {  // SolverControl::NoConvergence
  unsigned int last_step;
  double last_residual;
  NoConvergence(unsigned int s, double r) : std::runtime_error("Iterative method reported convergence failure"), last_step(s), last_residual(r) {}
};

// Function<dim>-like functor of the inlet profile (NavierStokes3D.hpp:17-81 / NavierStokes2D.hpp:18-81).
template <int dim>
class InletVelocity {
public:
  explicit InletVelocity(int test_case_ = 2, double u_m_ = dim == 3 ? 9.0 : 1.5) : test_case(test_case_), u_m(u_m_) {}
  void set_time(double t) { time = t; }
  double get_time() const { return time; }
  double value(const double *p, unsigned int component = 0) const {
    if (component != 0 || test_case == 1) return 0.0;
    if (dim == 3) {
      const double v = 16.0 * u_m * p[1] * p[2] * (H - p[2]) * (H - p[1]) / (H * H * H * H);
      return test_case == 3 ? 16.0 * u_m * p[1] * p[2] * (H - p[2]) * (H - p[1]) * std::sin(M_PI * time / 8.0) / (H * H * H * H) : v;
    }
    if (test_case == 2) return 4.0 * u_m * p[1] * (H - p[1]) * std::sin(M_PI * time / 8.0) / (H * H);  // NavierStokes2D.hpp:33-34
    return 4.0 * u_m * p[1] * (H - p[1]) / (H * H);
  }
  double getMeanVelocity() const {  // NavierStokes3D.hpp:64-75, NavierStokes2D.hpp:64-76
    if (test_case == 1) return 0.0;
    const double k = dim == 3 ? 4.0 / 9.0 : 2.0 / 3.0;
    return test_case == 3 ? k * u_m * std::sin(time * M_PI / 8.0) : k * u_m;
  }

protected:
  int test_case;
  double H = 0.41;
  double u_m;
  double time = 0.0;
};

template <int dim>
class NavierStokes {
public:
  // mesh_file_name: a gmsh .msh file, or "level:N" for the built-in cylinder generator (no .msh ships with the reference)
  NavierStokes(const std::string &mesh_file_name_, const unsigned int &degree_velocity_, const unsigned int &degree_pressure_,
               const double &T_, const double &deltat_, const int test_case_ = 2, const int n_ranks_ = 1,
               const double u_m_ = dim == 3 ? 9.0 : 1.5)  // u_m: a hard-coded member in the reference (NavierStokes3D.hpp:80: Re = 400); 2.25 gives Re = 100
      : test_case(test_case_), inlet_velocity(test_case_, u_m_), T(T_), mesh_file_name(mesh_file_name_), degree_velocity(degree_velocity_),
        degree_pressure(degree_pressure_), deltat(deltat_), n_ranks(n_ranks_) {
    if (degree_velocity != 2 || degree_pressure != 1) throw std::runtime_error("only Taylor-Hood P2/P1 is supported");
  }
  ~NavierStokes() {
    if (h) nsx_destroy(h);
    if (dofs) nsxh_dofs_free(dofs);
    if (mesh) nsxh_mesh_free(mesh);
  }

  std::vector<double> time_prec, time_solve;  // NavierStokes3D.hpp:121-122
  std::vector<double> vec_drag, vec_lift, vec_drag_coeff, vec_lift_coeff;  // NavierStokes3D.hpp:116-119 (never filled there)
  std::vector<int> gmres_iterations;
  bool write_output = true;   // output(): VTU + PVTU record every 20 steps (3D) / every step (2D), like the reference
  bool write_csv = true;      // 2D: gmres.csv and coeff_2.csv appended per step (NavierStokes2D.cpp:623-636,679-692)
  unsigned int preconditioner_type = dim == 3 ? 0 : 3;  // NavierStokes3D.cpp:562 / NavierStokes2D.cpp:547
  double nu = 1e-3;                                     // NavierStokes3D.hpp:162
  bool verbose = true;

  void setup() {  // NavierStokes3D.cpp:2-157
    out() << "Initializing the mesh" << std::endl;
    if (mesh_file_name.rfind("level:", 0) == 0)
      mesh = nsxh_mesh_cylinder_level(dim, std::stoi(mesh_file_name.substr(6)));
    else
      mesh = nsxh_mesh_read_msh(mesh_file_name.c_str());
    if (!mesh || nsxh_mesh_dim(mesh) != dim) throw std::runtime_error("cannot read mesh " + mesh_file_name);
    if (n_ranks > 1 && nsxh_mesh_partition(mesh, 1, n_ranks)) throw std::runtime_error("partition failed");
    out() << "  Number of elements = " << nsxh_mesh_n_cells(mesh) << std::endl;
    out() << "Initializing the finite element space" << std::endl;
    nsxh_tables *t = nsxh_tables_create(dim, 0, 0);
    out() << "  DoFs per cell              = " << (dim == 3 ? 34 : 15) << std::endl;
    out() << "  Quadrature points per cell = " << nsxh_tables_n_q(t) << std::endl;
    out() << "Initializing the DoF handler" << std::endl;
    dofs = nsxh_distribute_dofs_ordered(mesh, NSXH_ORDER_COLOUR);  // shallow per-rank ILU(0) dependency graphs
    n_u = nsxh_n_u(dofs);
    n_p = nsxh_n_p(dofs);
    out() << "  Number of DoFs: " << std::endl << "    velocity = " << n_u << std::endl << "    pressure = " << n_p << std::endl
          << "    total    = " << n_u + n_p << std::endl;
    out() << "Initializing the linear system" << std::endl;
    nsx_params p{dim, 0, nu, deltat};
    if (nsx_create(&p, &h)) throw std::runtime_error(nsx_last_error(nullptr));
    ck(nsx_set_tables(h, nsxh_tables_n_q(t), nsxh_tables_n_p2(t), nsxh_tables_n_p1(t), nsxh_tables_N2(t), nsxh_tables_dN2(t),
                      nsxh_tables_N1(t), nsxh_tables_weights(t)));
    nsxh_tables_free(t);
    ck(nsx_set_mesh(h, nsxh_mesh_n_cells(mesh), nsxh_dofs_per_cell(dofs), nsxh_cell_dofs(dofs), nsxh_cell_coords(dofs), n_u, n_p));
    if (n_ranks > 1) ck(nsx_set_ranks(h, nsxh_n_subdomains(dofs), nsxh_owned_u_ptr(dofs), nsxh_owned_p_ptr(dofs)));
    setup_force_faces();
    if (probes_csv) {  // opt-in (NSX_PROBES=1): the two pressure points of compute_pressure_difference, located once
      const double pts3[6] = {0.45, 0.2, 0.205, 0.55, 0.2, 0.205}, pts2[4] = {0.15, 0.2, 0.25, 0.2};
      ck(nsx_set_probes(h, 2, dim == 3 ? pts3 : pts2, -1.0));
    }
    if (n_tracers > 0) {  // opt-in (NSX_TRACERS=<n>): n seeds on a line across the channel upstream of the obstacle, located once
      std::vector<double> seeds((size_t)n_tracers * dim);
      for (int k = 0; k < n_tracers; ++k) {
        const double y = n_tracers > 1 ? 0.1 + 0.2 * k / (n_tracers - 1) : 0.2;  // the obstacle spans y in [0.15, 0.25]
        seeds[(size_t)k * dim] = dim == 3 ? 0.25 : 0.1;                         // its centre is at x = 0.5 (3D) / 0.2 (2D)
        seeds[(size_t)k * dim + 1] = y;
        if (dim == 3) seeds[(size_t)k * dim + 2] = 0.205;
      }
      ck(nsx_set_tracers(h, n_tracers, seeds.data(), -1.0));
    }
    if (!lattice_counts.empty()) setup_lattice();
    if (surface_csv) setup_surface();
  }

  void solve() {  // NavierStokes3D.cpp:687-741
    out() << "===============================================" << std::endl << "Applying the initial condition" << std::endl;
    std::vector<double> u0((size_t)n_u + n_p, 0.0);  // u_0 = ZeroFunction (NavierStokes3D.hpp:200)
    ck(nsx_set_solution(h, u0.data()));
    output(0, {0.0, 0.0});  // NavierStokes3D.cpp:699, NavierStokes2D.cpp:712
    unsigned int time_step = 0;
    double time = 0;
    while (time < T - 0.5 * deltat) {
      time += deltat;
      ++time_step;
      inlet_velocity.set_time(time);
      out() << "n = " << std::setw(3) << time_step << ", t = " << std::setw(5) << time << ":" << std::flush;
      if (time == deltat) assemble(time);
      else assemble_time_step(time);
      solve_time_step();
      current_time = time;
      if (diagnostics_csv) write_diagnostics(time_step, time);
      if (probes_csv) write_pressure_difference(time_step, time);
      if (n_tracers > 0) write_tracers(time_step, time);
      if (stats_first > 0 && time_step >= (unsigned int)stats_first) accumulate_statistics();
      if (surface_csv) write_surface_loads(time);
      // NavierStokes3D.cpp:725-726, as written: an EXACT floating-point comparison of the accumulated time with T - deltat (true or false
      // by the rounding of the additions; the reference's own run decides it the same way, so the mirror does not "repair" it)
      if (dim == 3 && time == T - deltat) compute_pressure_difference();
      // NavierStokes3D.cpp:728-733 (forces only after t = 0.1); NavierStokes2D.cpp:737-741 (every step)
      std::vector<double> coefficients = {0.0, 0.0};
      if (dim == 2 || time > 0.1) {
        coefficients = compute_forces();
        c_D_max = std::max(coefficients[0], c_D_max);
        c_L_min = std::min(coefficients[1], c_L_min);
      }
      if (time_step % (dim == 3 ? 20 : 1) == 0) output(time_step, coefficients);  // NavierStokes3D.cpp:734, NavierStokes2D.cpp:743
    }
    if (stats_open) write_statistics();
    out() << "===============================================" << std::endl
          << "Drag Coefficient Max ----->   " << c_D_max << std::endl
          << std::endl
          << "Lift Coefficient Min ----->   " << c_L_min << std::endl
          << "===============================================" << std::endl;
  }

  // NavierStokes::compute_forces (NavierStokes3D.cpp:744-846 / NavierStokes2D.cpp:752-859)
  std::vector<double> compute_forces() {
    out() << "===============================================" << std::endl << "Computing forces: " << std::endl;
    double drag = 0, lift = 0;
    ck(nsx_compute_forces(h, &drag, &lift));
    out() << "Drag :\t " << drag << " Lift :\t " << lift << std::endl;
    const double mean_v = inlet_velocity.getMeanVelocity();
    const double D = 0.1, H = 0.41, rho = 1.;
    const double den = dim == 3 ? rho * mean_v * mean_v * D * H : mean_v * mean_v * D;
    const double c_d = (2. * drag) / den, c_l = (2. * lift) / den;
    out() << "Coeff:\t " << c_d << " Coeff:\t " << c_l << std::endl;
    vec_drag.push_back(drag);
    vec_lift.push_back(lift);
    vec_drag_coeff.push_back(c_d);
    vec_lift_coeff.push_back(c_l);
    return {c_d, c_l};
  }

  // Not in the reference: energy, divergence, dissipation, enstrophy, change against previous_solution, CFL number and largest speed of
  // the state the handle holds, computed on the device (nsx_compute_diagnostics).  *numeric (optional): set when a value is not finite
  // (the struct is filled all the same); without it such a state throws like every other error.
  nsx_flow_diag compute_diagnostics(bool *numeric = nullptr) const {
    nsx_flow_diag d{};
    const int rc = nsx_compute_diagnostics(h, &d);
    if (numeric) *numeric = rc == NSX_ERR_NUMERIC;
    if (!(numeric && rc == NSX_ERR_NUMERIC)) ck(rc);
    return d;
  }

  // NavierStokes::output (NavierStokes3D.cpp:643-683; NavierStokes2D.cpp:642-695 also appends the coefficients to coeff_2.csv)
  void output(const unsigned int &time_step, const std::vector<double> &coeff = {0.0, 0.0}) const {
    if (write_output) {
      out() << "===============================================" << std::endl;
      const std::string output_file_name = dim == 3 ? "output-navier-stokes-3D" : "output-navier-stokes-2D";
      const std::vector<double> x = get_solution();
      const char *directory = dim == 3 ? "./outputConvergence/" : "./output2D_1/";
      if (fields_vtu) {  // opt-in (NSX_FIELDS=1): the same files with the nodal vorticity and Q-criterion of this state, computed on the device
        int n_vorticity = 0;
        ck(nsx_compute_nodal_fields(h));
        ck(nsx_nodal_field_components(h, NSX_FIELD_VORTICITY, &n_vorticity));
        std::vector<double> vorticity((size_t)(n_u / dim) * n_vorticity), q((size_t)(n_u / dim));
        ck(nsx_get_nodal_field(h, NSX_FIELD_VORTICITY, vorticity.data()));
        ck(nsx_get_nodal_field(h, NSX_FIELD_Q, q.data()));
        if (nsxh_write_vtu_fields(dofs, x.data(), vorticity.data(), n_vorticity, q.data(), directory, output_file_name.c_str(), time_step))
          throw std::runtime_error("cannot write " + output_file_name);
      } else if (nsxh_write_vtu(dofs, x.data(), directory, output_file_name.c_str(), time_step))
        throw std::runtime_error("cannot write " + output_file_name);
      if (!lattice_counts.empty()) write_lattice(time_step, directory);
      if (surface_csv) write_surface_distribution(time_step, directory);
      out() << "Output written to " << output_file_name << std::endl;
    }
    if (dim == 2 && write_csv) {
      std::ofstream coeff_file("coeff_2.csv", std::ios::app);
      if (coeff_file.is_open()) coeff_file << time_step << "," << coeff[0] << "," << coeff[1] << "\n";
      else out() << "Error: Unable to open coeff.csv for writing." << std::endl;
    }
    if (write_output) out() << "===============================================" << std::endl;
  }

  // NavierStokes::compute_pressure_difference (NavierStokes3D.cpp:849-923)
  double compute_pressure_difference() const {
    const double p_a[3] = {0.45, 0.2, 0.205}, p_e[3] = {0.55, 0.2, 0.205};
    const std::vector<double> x = get_solution();
    double p_diff = 0.0;
    nsxh_pressure_difference(dofs, x.data(), p_a, p_e, &p_diff);
    out() << "Pressure difference (P(A) - P(B)) = " << p_diff << std::endl;
    return p_diff;
  }
  double c_D_max = -999, c_L_min = 999;

  std::vector<double> get_solution() const {
    std::vector<double> x((size_t)n_u + n_p);
    if (nsx_get_solution(h, x.data())) throw std::runtime_error(nsx_last_error(h));
    return x;
  }

protected:
  void assemble(const double &time) {  // NavierStokes3D.cpp:163-356
    out() << "===============================================" << std::endl << "Assembling the system" << std::endl;
    ck(nsx_assemble(h, NSX_TEMAM));
    apply_dirichlet(time);
  }
  void assemble_time_step(const double &time) {  // NavierStokes3D.cpp:361-544 (Temam kept in 2D: NavierStokes2D.cpp:446)
    out() << "===============================================" << std::endl << "Assembling the system" << std::endl;
    ck(nsx_assemble_time_step(h, dim == 2 ? NSX_TEMAM : 0));
    apply_dirichlet(time);
  }
  void apply_dirichlet(const double &time) {  // NavierStokes3D.cpp:327-354, 515-542
    std::map<int32_t, double> boundary_values;
    inlet_velocity.set_time(time);
    const double *sp = nsxh_support_points(dofs);
    const int32_t *d;
    int n = nsxh_boundary_dofs(dofs, 0, &d);
    for (int k = 0; k < n; ++k) boundary_values[d[k]] = inlet_velocity.value(sp + (size_t)d[k] * dim, d[k] % dim);
    for (int id : {2, 3}) {  // zero_function on walls and obstacle; overwrites shared dofs like the second interpolate_boundary_values
      n = nsxh_boundary_dofs(dofs, id, &d);
      for (int k = 0; k < n; ++k) boundary_values[d[k]] = 0.0;
    }
    std::vector<int32_t> bd;
    std::vector<double> bv;
    for (const auto &kv : boundary_values) {
      bd.push_back(kv.first);
      bv.push_back(kv.second);
    }
    ck(nsx_apply_boundary_values(h, (int)bd.size(), bd.data(), bv.data()));
  }
  void solve_time_step() {  // NavierStokes3D.cpp:546-640
    out() << "===============================================" << std::endl;
    if (preconditioner_type > 3) throw std::runtime_error("Invalid preconditioner type");  // NavierStokes3D.cpp:633
    nsx_solve_stats st;
    const unsigned int inner_maxiter = (preconditioner_type == 1 || preconditioner_type == 3) ? 10000 : 100000;  // Preconditioners.hpp:155,259,368,482
    const int rc = nsx_solve_time_step(h, (int)preconditioner_type, 1e-4, 1e-2, 100000, (int)inner_maxiter, &st);
    if (rc == NSX_ERR_NOCONV) throw NoConvergence(st.outer_iterations, st.final_residual);
    ck(rc);
    out() << "Time taken to initialize preconditioner: " << st.t_prec << " seconds" << std::endl;
    out() << "Time taken to solve Navier Stokes problem: " << st.t_solve << " seconds" << std::endl;
    time_prec.push_back(st.t_prec);
    time_solve.push_back(st.t_solve);
    gmres_iterations.push_back(st.outer_iterations);
    if (gmres_iterations.size() == 1) {  // once: which inner precision the handle runs (nsx_set_inner_precision / NSX_INNER_PRECISION), from the first solve's paths
      int info[32];
      ck(nsx_path_info(h, info));
      out() << "nsx: inner precision " << (info[26] || info[27] ? "FP32" : "FP64") << " (float values in the inner F products " << info[26] << ", in the velocity triangular solves " << info[27] << ")" << std::endl;
    }
    out() << "Result:  " << st.outer_iterations << " GMRES iterations" << std::endl;
    if (dim == 2 && write_csv) {  // NavierStokes2D.cpp:622-636
      const int Re = int(0.1 * 1.5 * std::sin(inlet_velocity.get_time() * M_PI / 8.0) / .001);
      std::ofstream coeff_file("gmres.csv", std::ios::app);
      if (coeff_file.is_open()) coeff_file << inlet_velocity.get_time() << ',' << Re << ',' << st.outer_iterations << "\n";
      else out() << "Error: Unable to open coeff.csv for writing." << std::endl;
    }
  }

  // opt-in monitor (NSX_DIAGNOSTICS=1): one row per time step in diagnostics_{2D,3D}.csv; a state that is not finite ends the run behind its row
  void write_diagnostics(const unsigned int time_step, const double time) const {
    bool numeric = false;
    const nsx_flow_diag d = compute_diagnostics(&numeric);
    char row[512];
    snprintf(row, sizeof(row), "%u,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g\n", time_step, time, d.kinetic_energy, d.div_l2, d.grad_l2_sq,
             d.enstrophy, d.change_l2, d.cfl_max, d.speed_max);
    std::ofstream file(dim == 3 ? "diagnostics_3D.csv" : "diagnostics_2D.csv", std::ios::app);
    if (!file.is_open()) throw std::runtime_error("cannot write the diagnostics file");
    file << row;
    if (numeric) throw std::runtime_error(std::string("nsx: ") + nsx_last_error(h));
  }

  // opt-in series (NSX_PROBES=1): p(A), p(E) and p(A) - p(E) of every time step in pressure_difference_{2D,3D}.csv, evaluated on the device
  // (nsx_eval_probes); compute_pressure_difference itself stays on the front-end path
  void write_pressure_difference(const unsigned int time_step, const double time) const {
    double p[2] = {0.0, 0.0};
    ck(nsx_eval_probes(h, nullptr, p, nullptr, nullptr));
    char row[256];
    snprintf(row, sizeof(row), "%u,%.17g,%.17g,%.17g,%.17g\n", time_step, time, p[0], p[1], p[0] - p[1]);
    std::ofstream file(dim == 3 ? "pressure_difference_3D.csv" : "pressure_difference_2D.csv", std::ios::app);
    if (!file.is_open()) throw std::runtime_error("cannot write the pressure difference file");
    file << row;
  }

  // opt-in series (NSX_TRACERS=<n>): the particles are carried through the step just solved (RK4, the field interpolated linearly in time
  // from previous_solution to solution, 4 substeps) and one row per particle is appended to tracers_{2D,3D}.csv:
  // step, time, particle, x, y[, z], cell, status, exit face, age
  void write_tracers(const unsigned int time_step, const double time) const {
    ck(nsx_advect_tracers(h, deltat, 4, NSX_TRACER_RK4, NSX_TRACER_LINEAR));
    std::vector<double> x((size_t)n_tracers * dim), age(n_tracers);
    std::vector<int32_t> cell(n_tracers), status(n_tracers), face(n_tracers);
    ck(nsx_get_tracers(h, x.data(), cell.data(), status.data(), face.data(), age.data()));
    std::ofstream file(dim == 3 ? "tracers_3D.csv" : "tracers_2D.csv", std::ios::app);
    if (!file.is_open()) throw std::runtime_error("cannot write the tracer file");
    char row[320];
    for (int k = 0; k < n_tracers; ++k) {
      int n = snprintf(row, sizeof(row), "%u,%.17g,%d", time_step, time, k);
      for (int d = 0; d < dim; ++d) n += snprintf(row + n, sizeof(row) - n, ",%.17g", x[(size_t)k * dim + d]);
      snprintf(row + n, sizeof(row) - n, ",%d,%d,%d,%.17g\n", cell[k], status[k], face[k], age[k]);
      file << row;
    }
  }

  // opt-in statistics (NSX_STATS=<first step>): from that time step on velocity and pressure of every step go into one running mean and
  // co-moment on the device with weight deltat (nsx_stats_accumulate, one launch per step, nothing is downloaded) ...
  void accumulate_statistics() {
    if (!stats_open) ck(nsx_stats_begin(h, NSX_STATS_VELOCITY | NSX_STATS_PRESSURE, 1));
    stats_open = true;
    ck(nsx_stats_accumulate(h, 0, deltat));
  }

  // ... and after the last step the time-averaged flow is written to stats_{2D,3D}.vtu: mean velocity, mean pressure, rms velocity, the
  // Reynolds stresses and the turbulent kinetic energy
  void write_statistics() const {
    const size_t n_nodes = (size_t)(n_u / dim), nsym = (size_t)dim * (dim + 1) / 2;
    std::vector<double> mean_u(n_nodes * dim), mean_p((size_t)n_p), rms_u(n_nodes * dim), stress(n_nodes * nsym), tke(n_nodes);
    ck(nsx_stats_get(h, NSX_STATS_MEAN_U, 0, mean_u.data()));
    ck(nsx_stats_get(h, NSX_STATS_MEAN_P, 0, mean_p.data()));
    ck(nsx_stats_get(h, NSX_STATS_RMS_U, 0, rms_u.data()));
    ck(nsx_stats_get(h, NSX_STATS_STRESS_U, 0, stress.data()));
    ck(nsx_stats_get(h, NSX_STATS_TKE, 0, tke.data()));
    if (nsxh_write_vtu_stats(dofs, mean_u.data(), mean_p.data(), rms_u.data(), stress.data(), tke.data(), "./", dim == 3 ? "stats_3D" : "stats_2D"))
      throw std::runtime_error("cannot write the statistics file");
    int64_t samples = 0;
    ck(nsx_stats_info(h, nullptr, nullptr, &samples, nullptr));
    out() << "Statistics of " << samples << " time steps written to " << (dim == 3 ? "stats_3D.vtu" : "stats_2D.vtu") << std::endl;
  }

  // opt-in image (NSX_LATTICE="nx,ny[,nz]"): a lattice of that many points spanning the bounding box of the mesh, located once
  void setup_lattice() {
    if ((int)lattice_counts.size() != dim) throw std::runtime_error("NSX_LATTICE: " + std::to_string(dim) + " counts of at least 1, separated by commas");
    const double *X = nsxh_cell_coords(dofs);
    const size_t n_vertices = (size_t)nsxh_mesh_n_cells(mesh) * (dim + 1);
    for (int d = 0; d < dim; ++d) {
      double lo = X[d], hi = X[d];
      for (size_t v = 1; v < n_vertices; ++v) {
        lo = std::min(lo, X[v * dim + d]);
        hi = std::max(hi, X[v * dim + d]);
      }
      const int32_t n = lattice_counts[d];
      lattice_origin[d] = n > 1 ? lo : (lo + hi) / 2;
      lattice_spacing[d] = n > 1 ? (hi - lo) / (n - 1) : 1.0;
    }
    ck(nsx_set_lattice(h, lattice_origin, lattice_spacing, lattice_counts.data(), -1.0, nullptr));
  }

  // ... and at every output() velocity, pressure and, with NSX_FIELDS=1, the vorticity of the state are sampled on it on the device and
  // written beside the VTU as lattice-navier-stokes-{2D,3D}_<step>.vti, with the owner cells as the mask "cell_id"
  void write_lattice(const unsigned int time_step, const char *directory) const {
    size_t n = 1;
    for (const int32_t c : lattice_counts) n *= (size_t)c;
    const int n_vorticity = dim == 3 ? 3 : 1;
    std::vector<double> velocity(n * dim), pressure(n), vorticity(fields_vtu ? n * n_vorticity : 0);
    std::vector<int32_t> cells(n);
    ck(nsx_eval_lattice(h, NSX_LATTICE_VELOCITY | NSX_LATTICE_PRESSURE | (fields_vtu ? NSX_LATTICE_NODAL : 0)));  // output() has computed the nodal fields
    ck(nsx_get_lattice(h, NSX_LATTICE_VELOCITY, 0, velocity.data()));
    ck(nsx_get_lattice(h, NSX_LATTICE_PRESSURE, 0, pressure.data()));
    if (fields_vtu) ck(nsx_get_lattice(h, NSX_LATTICE_NODAL, NSX_FIELD_VORTICITY, vorticity.data()));
    ck(nsx_get_lattice_cells(h, cells.data()));
    if (nsxh_write_vti(dim, lattice_origin, lattice_spacing, lattice_counts.data(), velocity.data(), pressure.data(), cells.data(),
                       fields_vtu ? vorticity.data() : nullptr, n_vorticity, directory, dim == 3 ? "lattice-navier-stokes-3D" : "lattice-navier-stokes-2D", time_step))
      throw std::runtime_error("cannot write the lattice file");
  }

  // opt-in surface loads (NSX_SURFACE=1): every boundary face, grouped by boundary id 0 .. 3 (inlet, outlet, walls, obstacle), symmetric
  // viscous stress, torque about the cylinder's axis; installed once (nsx_set_surface)
  void setup_surface() {
    const int nbf = nsxh_mesh_n_bfaces(mesh);
    const int32_t *ids = nsxh_mesh_bface_ids(mesh), *bc = nsxh_mesh_bface_cells(mesh);
    std::vector<int32_t> fc, fl, fg;
    for (int f = 0; f < nbf; ++f) {
      if (ids[f] < 0 || ids[f] > 3) continue;
      fc.push_back(bc[f]);
      fl.push_back(local_face(f));
      fg.push_back(ids[f]);
    }
    const double axis3[3] = {0.5, 0.2, 0.205}, axis2[2] = {0.2, 0.2};
    ck(nsx_set_surface(h, (int)fc.size(), fc.data(), fl.data(), fg.data(), 4, NSX_SURFACE_SYMMETRIC, dim == 3 ? axis3 : axis2));
    std::ofstream file(dim == 3 ? "surface_loads_3D.csv" : "surface_loads_2D.csv", std::ios::trunc);  // a run starts its series anew
    if (!file.is_open()) throw std::runtime_error("cannot write the surface loads file");
  }

  // ... every time step appends to surface_loads_{2D,3D}.csv: time, pressure force [dim], viscous force [dim] and torque [3 | 1] on the
  // obstacle, flow rate through the inlet, flow rate through the outlet (nsx_compute_surface: one fold on the device, 4 groups downloaded)
  void write_surface_loads(const double time) const {
    nsx_surface_totals t[4];
    ck(nsx_compute_surface(h, t));
    char row[640];
    int n = snprintf(row, sizeof(row), "%.17g", time);
    for (int d = 0; d < dim; ++d) n += snprintf(row + n, sizeof(row) - n, ",%.17g", t[3].force_pressure[d]);
    for (int d = 0; d < dim; ++d) n += snprintf(row + n, sizeof(row) - n, ",%.17g", t[3].force_viscous[d]);
    for (int d = dim == 3 ? 0 : 2; d < 3; ++d) n += snprintf(row + n, sizeof(row) - n, ",%.17g", t[3].torque[d]);
    snprintf(row + n, sizeof(row) - n, ",%.17g,%.17g\n", t[0].flux, t[1].flux);
    std::ofstream file(dim == 3 ? "surface_loads_3D.csv" : "surface_loads_2D.csv", std::ios::app);
    if (!file.is_open()) throw std::runtime_error("cannot write the surface loads file");
    file << row;
  }

  // ... and every output() writes surface-navier-stokes-{2D,3D}_<step>.csv beside the VTU, one row per surface node of the obstacle:
  // position [dim], normal [dim], pressure, wall shear stress [dim]
  void write_surface_distribution(const unsigned int time_step, const char *directory) const {
    int info[4];
    ck(nsx_surface_info(h, info));
    const size_t ns = (size_t)info[2];
    std::vector<int32_t> nodes(ns), groups(ns);
    std::vector<double> normal(ns * dim), pressure(ns), shear(ns * dim);
    ck(nsx_get_surface_layout(h, nodes.data(), groups.data(), nullptr, nullptr));
    ck(nsx_compute_surface(h, nullptr));
    ck(nsx_get_surface_field(h, NSX_SURFACE_NORMAL, NSX_SURFACE_AT_NODES, normal.data()));
    ck(nsx_get_surface_field(h, NSX_SURFACE_PRESSURE, NSX_SURFACE_AT_NODES, pressure.data()));
    ck(nsx_get_surface_field(h, NSX_SURFACE_SHEAR, NSX_SURFACE_AT_NODES, shear.data()));
    std::ofstream file(std::string(directory) + (dim == 3 ? "surface-navier-stokes-3D_" : "surface-navier-stokes-2D_") + std::to_string(time_step) + ".csv");
    if (!file.is_open()) throw std::runtime_error("cannot write the surface distribution file");
    const double *sp = nsxh_support_points(dofs);
    char row[640];
    for (size_t s = 0; s < ns; ++s) {
      if (groups[s] != 3) continue;
      int n = 0;
      for (int d = 0; d < dim; ++d) n += snprintf(row + n, sizeof(row) - n, "%.17g,", sp[(size_t)nodes[s] * dim * dim + d]);  // velocity dof dim * node
      for (int d = 0; d < dim; ++d) n += snprintf(row + n, sizeof(row) - n, "%.17g,", normal[s * dim + d]);
      n += snprintf(row + n, sizeof(row) - n, "%.17g", pressure[s]);
      for (int d = 0; d < dim; ++d) n += snprintf(row + n, sizeof(row) - n, ",%.17g", shear[s * dim + d]);
      file << row << "\n";
    }
  }

  static std::vector<int32_t> parse_counts(const char *text) {  // "nx,ny[,nz]"; anything else: one entry 0, which setup_lattice refuses
    std::vector<int32_t> counts;
    if (!text || !*text) return counts;
    std::stringstream in(text);
    std::string item;
    while (std::getline(in, item, ',')) {
      char *end = nullptr;
      const long v = std::strtol(item.c_str(), &end, 10);
      counts.push_back(end != item.c_str() && *end == 0 && v >= 1 && v <= (1 << 26) ? (int32_t)v : 0);
    }
    for (const int32_t c : counts)
      if (c == 0) return std::vector<int32_t>(4, 0);
    return counts;
  }

  int local_face(const int f) const {  // deal.II local face number of boundary face f in its cell (-1: none, which libnsx refuses)
    static const int TETF[4][3] = {{0, 1, 2}, {1, 0, 3}, {0, 2, 3}, {2, 1, 3}};
    static const int TRIF[3][2] = {{0, 1}, {1, 2}, {2, 0}};
    const int32_t *bf = nsxh_mesh_bfaces(mesh), *cv = nsxh_mesh_cells(mesh) + (size_t)nsxh_mesh_bface_cells(mesh)[f] * (dim + 1);
    for (int lf = 0; lf <= dim; ++lf) {
      int match = 0;
      for (int k = 0; k < dim; ++k) {
        const int32_t v = cv[dim == 3 ? TETF[lf][k] : TRIF[lf][k]];
        for (int q = 0; q < dim; ++q) match += v == bf[(size_t)f * dim + q];
      }
      if (match == dim) return lf;
    }
    return -1;
  }

  void setup_force_faces() {  // faces with boundary id 3 and the face-quadrature tables (FEFaceValues of compute_forces)
    const int nbf = nsxh_mesh_n_bfaces(mesh);
    const int32_t *ids = nsxh_mesh_bface_ids(mesh), *bc = nsxh_mesh_bface_cells(mesh);
    std::vector<int32_t> fc, fl;
    for (int f = 0; f < nbf; ++f) {
      if (ids[f] != 3) continue;
      const int lf = local_face(f);
      if (lf < 0) continue;
      fc.push_back(bc[f]);
      fl.push_back(lf);
    }
    nsxh_tables *t = nsxh_tables_create(dim, 1, 0);
    ck(nsx_set_force_faces(h, (int)fc.size(), fc.data(), fl.data(), nsxh_tables_n_qf(t), nsxh_tables_N2(t), nsxh_tables_dN2(t),
                           nsxh_tables_N1(t), nsxh_tables_weights(t)));
    nsxh_tables_free(t);
  }

  void ck(int rc) const {
    if (rc) throw std::runtime_error(std::string("nsx: ") + nsx_last_error(h));
  }
  std::ostream &out() const {
    static std::ofstream null;
    return verbose ? std::cout : null;
  }

  unsigned int test_case;
  InletVelocity<dim> inlet_velocity;
  const double T;
  const std::string mesh_file_name;
  const unsigned int degree_velocity, degree_pressure;
  const double deltat;
  const int n_ranks;
  nsxh_mesh *mesh = nullptr;
  nsxh_dofs *dofs = nullptr;
  nsx_handle *h = nullptr;
  int n_u = 0, n_p = 0;
  double current_time = 0.0;
  const bool diagnostics_csv = std::getenv("NSX_DIAGNOSTICS") && std::string(std::getenv("NSX_DIAGNOSTICS")) == "1";
  const bool probes_csv = std::getenv("NSX_PROBES") && std::string(std::getenv("NSX_PROBES")) == "1";
  const bool fields_vtu = std::getenv("NSX_FIELDS") && std::string(std::getenv("NSX_FIELDS")) == "1";
  const std::vector<int32_t> lattice_counts = parse_counts(std::getenv("NSX_LATTICE"));
  static bool surface_wanted() {  // NSX_SURFACE: unset = off, 1 = on, anything else is an error
    const char *e = std::getenv("NSX_SURFACE");
    if (e && std::string(e) != "1") throw std::runtime_error("NSX_SURFACE: set it to 1 to write the surface loads, or leave it unset (got \"" + std::string(e) + "\")");
    return e != nullptr;
  }
  const bool surface_csv = surface_wanted();
  double lattice_origin[3] = {0.0, 0.0, 0.0}, lattice_spacing[3] = {1.0, 1.0, 1.0};
  const int stats_first = std::getenv("NSX_STATS") ? std::max(0, std::atoi(std::getenv("NSX_STATS"))) : 0;  // first time step of the statistics (0: none)
  bool stats_open = false;
  const int n_tracers = std::getenv("NSX_TRACERS") ? std::max(0, std::min(1048576, std::atoi(std::getenv("NSX_TRACERS")))) : 0;
};

}  // namespace nsx
