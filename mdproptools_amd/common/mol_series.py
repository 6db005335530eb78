"""
What the drop-in modules over per-molecule series share (dynamical/reorientation.py, structural/dihedral_distribution.py):
the molecule layout and its jobs, the loader that reduces the dumps batch by batch to the series U [S,3,F] on the device,
and the checks in front of `backend.orient_corr`. A JOB covers every molecule of one type; jobs add to ROWS (a vector, or
a dihedral entry that pools several quadruples), and a row is one group of series.
"""

import numpy as np

from . import trajectory as T


def layout(num_mols, num_atoms_per_mol):
    """(molecules per type, atoms per molecule) as lists of int, one entry per molecule type."""
    num_mols, per = [int(v) for v in num_mols], [int(v) for v in num_atoms_per_mol]
    if len(num_mols) != len(per):
        raise ValueError("num_mols and num_atoms_per_mol must hold one entry per molecule type")
    return num_mols, per


def type_jobs(types, num_mols, num_atoms_per_mol):
    """(job_atom0 int64, job_mols int64, job_len int32) of one job per entry of `types` (0-based molecule types, in id
    order): all molecules of the type, from the type's first atom on."""
    first = np.concatenate(([0], np.cumsum(np.multiply(num_mols, num_atoms_per_mol)))).astype(np.int64)
    return (first[types], np.asarray([num_mols[t] for t in types], dtype=np.int64),
            np.asarray([num_atoms_per_mol[t] for t in types], dtype=np.int32))


def same_rows(col, start, m, n, what, label):
    """Row [n] that the m molecules of n atoms from atom `start` on share in the per-atom column `col` (charges,
    types), or a ValueError."""
    rows = np.asarray(col[start:start + m * n], dtype=np.float64).reshape(m, n)
    if m and np.any(rows != rows[0]):
        raise ValueError("species %s: the molecules of the type do not all carry the same %s" % (label, what))
    return rows[0] if m else np.zeros(n)


def load_series(filename, coords, n_atoms, compute, job_mols, job_rows, n_rows, dt=None, lead="id", **how):
    """Reduces the frames of `filename` batch by batch (trajectory.attribute_batches; `how`: its stream, batch_bytes,
    missing): compute(xyz, box, out, ctx, first) — box None unless coords is "wrapped", first the batch's `lead` column
    — writes the batch's series into `out` (float64 CUDA tensor [S,3,B], S = sum(job_mols)) and returns the degenerate
    count of every job. -> (U [S,3,F] float64 CUDA tensor with the frames in time order, times [F] in ps (dt: ps per
    timestep unit), group_off int64 [n_rows+1]: the series of row r are those of the jobs with job_rows == r,
    degenerate uint64 [n_rows]). dt None: counts only — out, ctx, U and times are None, nothing is asked of the
    timesteps."""
    from .. import backend

    if dt is not None:
        import torch
    wrapped = coords == "wrapped"
    _, batches = T.attribute_batches(filename, (lead, "type"), ["x", "y", "z"] if wrapped else T.UNWRAPPED,
                                     n_atoms=n_atoms, with_box=True, **how)
    S = int(np.sum(job_mols))
    out = ctx = None
    parts, steps = [], []
    degenerate = np.zeros(n_rows, dtype=np.uint64)
    # whatever the route, each batch is reduced to series [S,3,B] that stay on the device
    for ts, first, _types, xyz, box in batches:
        if dt is not None:
            ctx = ctx or backend.default_context()
            out = torch.empty((S, 3, len(ts)), dtype=torch.float64, device=torch.device("cuda", ctx.device))
        np.add.at(degenerate, job_rows, np.asarray(compute(xyz, box if wrapped else None, out, ctx, first), dtype=np.uint64))
        parts.append(out)
        steps.extend(np.asarray(ts).tolist())
    if not parts:
        raise ValueError(f"no frames match {filename}")
    group_off = np.concatenate(([0], np.cumsum(np.bincount(job_rows, job_mols, n_rows)))).astype(np.int64)
    if dt is None:
        return None, None, group_off, degenerate
    from ..dynamical.conductivity import Conductivity

    order, times = Conductivity.frame_times(steps, dt)
    U = parts[0] if len(parts) == 1 else torch.cat(parts, dim=2)
    if np.any(order != np.arange(len(order))):
        U = U.index_select(2, torch.as_tensor(order, device=U.device))
    return U.contiguous(), times, group_off, degenerate


def refuse_degenerate(labels, degenerate, what, why):
    """ValueError that names the rows with a degenerate count: what does not exist has no correlation function."""
    if np.any(degenerate):
        bad = ", ".join("%s (%d)" % (lab, n) for lab, n in zip(labels, degenerate) if n)
        raise ValueError("%s (in brackets: molecule-frame pairs): %s. %s" % (what, bad, why))


def orient_corr(U, group_off, max_lag):
    """(max_lag, sums [max_lag+1,G,2] of backend.orient_corr) over U [S,3,F]; max_lag defaults to (F - 1) // 2."""
    from .. import backend

    F = U.shape[2]
    max_lag = (F - 1) // 2 if max_lag is None else int(max_lag)
    if not 0 <= max_lag <= F - 1:
        raise ValueError("max_lag must be in [0, n_frames - 1 = %d]" % (F - 1))
    return max_lag, backend.orient_corr(U, group_off, max_lag)
