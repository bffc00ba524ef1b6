// fd_ode.h -- host side of the probability-flow ODE sampler (fd_ode.hip): the per-evaluation coefficient table and the
// step-by-step stage launch shared by the three loop forms (persistent kernel, long-series fused launch, per-op launches).
#pragma once
#include <vector>

#include "fd_common.h"
#include "fd_mega_params.h"

// Rows of the Euler (n_steps rows) or Heun (2 n_steps rows: predictor at t_i, corrector at t_{i+1}) loop over the grid
// timesteps[0 .. n_steps] (host).  FD_ERR_ARG unless the grid is finite and strictly monotone.
int fd_ode_table(fd_ctx* ctx, const fd_sde_params* sde, const float* timesteps, int n_steps, int solver,
                 std::vector<fd_ode_step_coef>* rows);
// Rows of the data-prediction solvers (fd_mega_params.h) over a sampling grid: solver 2 = DDIM (first order), 3 = DPM-Solver++ 2M;
// one row and one fd_dpm_coef per step, computed in double.  FD_ERR_ARG unless the grid is finite, strictly decreasing, and the
// log-SNR lambda = log(alpha / s) strictly increasing along it.
int fd_dpm_table(fd_ctx* ctx, const fd_sde_params* sde, const float* timesteps, int n_steps, int solver,
                 std::vector<fd_ode_step_coef>* rows, std::vector<fd_dpm_coef>* dpm);
// The table of solver 0 Euler, 1 Heun (fd_ode_table), 2 DDIM, 3 DPM-Solver++ 2M (fd_dpm_table; *dpm stays empty for 0 and 1) and
// the number of (B,T,C) state buffers its step-by-step loop keeps: Heun 2, DPM-Solver++ 2M 1, else 0.
int fd_solver_rows(fd_ctx* ctx, const fd_sde_params* sde, const float* timesteps, int n_steps, int solver,
                   std::vector<fd_ode_step_coef>* rows, std::vector<fd_dpm_coef>* dpm, int* nstate);
// x <- stage(x, score) in place on (B,T,C); x0 / v0: the Heun state, (B,T,C) each (not read for FD_ODE_EULER).  Data-prediction
// stages (FD_ODE_DDIM and above): w is their second coefficient pair and x0 holds D_prev (not touched by FD_ODE_DDIM).  A paired
// guide g (fd_loop.h): x and score are (2B,T,C), the stage runs on the guided score and writes both halves of x.
struct fd_guide;
int fd_ode_stage(fd_ctx* ctx, const float* G, float* x, const float* score, float* x0, float* v0, const fd_ode_step_coef& c,
                 int B, int T, int C, hipStream_t s, const fd_dpm_coef* w = nullptr, const fd_guide* g = nullptr);
// the loop forms of fd_score_bf16.hip; FD_ERR_UNSUPPORTED (x untouched) when the model / shape has no such path.  dpm: the
// data-prediction solvers' second coefficient pair of every row, or null (Euler / Heun)
int fd_sampler_run_ode_mega(fd_score* m, const std::vector<fd_ode_step_coef>& rows, const float* G, float* x, int B, hipStream_t s,
                            const std::vector<fd_dpm_coef>* dpm = nullptr);
int fd_sampler_run_ode_layers(fd_score* m, const std::vector<fd_ode_step_coef>& rows, const float* G, float* x, int B, hipStream_t s,
                              const std::vector<fd_dpm_coef>* dpm = nullptr);
