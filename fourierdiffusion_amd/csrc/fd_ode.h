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
// x <- stage(x, score) in place on (B,T,C); x0 / v0: the Heun state, (B,T,C) each (not read for FD_ODE_EULER)
int fd_ode_stage(fd_ctx* ctx, const float* G, float* x, const float* score, float* x0, float* v0, const fd_ode_step_coef& c,
                 int B, int T, int C, hipStream_t s);
// the loop forms of fd_score_bf16.hip; FD_ERR_UNSUPPORTED (x untouched) when the model / shape has no such path
int fd_sampler_run_ode_mega(fd_score* m, const std::vector<fd_ode_step_coef>& rows, const float* G, float* x, int B, hipStream_t s);
int fd_sampler_run_ode_layers(fd_score* m, const std::vector<fd_ode_step_coef>& rows, const float* G, float* x, int B, hipStream_t s);
