// shape_plan.h — the runs of one mdhip_mol_shape call (mol_shape.hip): which molecules a workgroup owns and which of the
// two forms of the kernel works them, decided from the job table alone.
//
// A JOB covers job_mols molecules of job_len atoms from atom job_atom0 on (one molecule type). A RUN is a stretch of
// whole molecules of ONE job that a workgroup works at every frame of its slice:
//   staged (job_len <= SH_CAP): at most SH_MOLS molecules and at most SH_CAP atoms — what one LDS stage holds; the
//     workgroup loads the run's three planes with full-width loads and one lane per molecule walks its atoms in LDS;
//   walk (job_len > SH_CAP): SH_MOLS molecules, one lane each, walking global memory.
// Runs never cross a job: a workgroup's weights, end atoms, mass sum and histogram rows are uniform.
// Everything here is host arithmetic on plain values (no HIP header, no context), in the form of seg_plan.h:
// tests/native/shape_plan_main.cpp includes this header with g++ and walks it under sanitizers. An unnamed namespace, as
// the kernels that take ShRun: their symbols keep their names.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "mol_tile.h"  // (mol_jobs: the job walk and its errors)

namespace {

constexpr int SH_CAP = 1024;   // atoms per LDS stage
constexpr int SH_MOLS = 256;   // molecules per run at most = threads per workgroup
constexpr long long SH_MAX_RUNS = 1ll << 22;

struct ShRun {
    long long m0;  // first molecule of the run inside its job
    int job, nm;   // the job (call order) and the molecules of the run
};

// The job walk of mol_tile.h (mol_jobs: range, series0, 2^40) with one more RESULT rule: the runs reach 2^22 — a run
// table of 64 MiB. A refused plan holds no run.
struct ShPlan : MolJobs {
    std::vector<ShRun> staged, walk;  // job after job, molecules ascending
};

// molecules per run of a job of `len` atoms, and whether the run is staged
inline int sh_run_mols(long long len) { return len > SH_CAP ? SH_MOLS : (int)(SH_CAP / len < SH_MOLS ? SH_CAP / len : SH_MOLS); }

inline ShPlan shape_plan(int n_jobs, const int64_t *job_atom0, const int64_t *job_mols, const int32_t *job_len,
                         int64_t n_atoms, int64_t n_frames)
{
    ShPlan pl;
    long long runs = 0;
    mol_jobs(pl, n_jobs, job_atom0, job_mols, job_len, n_atoms, n_frames, [&](int, long long, long long mols, long long len) {
        const int per = sh_run_mols(len);
        runs += (mols + per - 1) / per;
        return runs < SH_MAX_RUNS;
    });
    if (pl.error != MOL_PLAN_OK) return pl;
    for (int j = 0; j < n_jobs; ++j) {
        const long long len = job_len[j], mols = job_mols[j];
        const int per = sh_run_mols(len);
        std::vector<ShRun> &to = len > SH_CAP ? pl.walk : pl.staged;
        for (long long m0 = 0; m0 < mols; m0 += per) to.push_back({m0, j, (int)(mols - m0 < per ? mols - m0 : per)});
    }
    return pl;
}

// Frame slices (gridDim.y) of a launch over `runs` runs: a workgroup takes the frames y, y + slices, ... About SH_FRAMES
// frames per workgroup, over which it zeroes and flushes its histogram row once and fetches the next frame while it works
// this one; more slices when the runs alone would not fill the chip several times over; never more than gridDim.y
// holds, nor than there are frames.
constexpr long long SH_FRAMES = 16, SH_MAX_GRID_Y = 65535;
inline unsigned shape_frame_slices(long long runs, int64_t n_frames, int cu_count)
{
    const long long fill = runs > 0 ? ((long long)cu_count * 16 + runs - 1) / runs : 1;
    const long long want = std::max(fill, ((long long)n_frames + SH_FRAMES - 1) / SH_FRAMES);
    return (unsigned)std::max<long long>(1, std::min({want, (long long)n_frames, SH_MAX_GRID_Y}));
}

// Sums that do not depend on the frame, on the host in index order from 0.0 (as seg_sums of seg_plan.h): the mass sum
// of one molecule of every job from its weight row w[w_off[j] .. w_off[j] + job_len[j])
inline std::vector<double> shape_mass_sums(int n_jobs, const int32_t *job_len, const int64_t *w_off, const double *w)
{
    std::vector<double> sums((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        double m = 0.0;
        for (int k = 0; k < job_len[j]; ++k) m += w[w_off[j] + k];
        sums[(size_t)j] = m;
    }
    return sums;
}

}  // namespace
