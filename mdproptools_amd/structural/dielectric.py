"""
The static dielectric constant from the fluctuation of the total dipole moment M of the cell (conducting boundary
conditions, as Ewald / PPPM runs have),

    eps_r = 1 + (<M . M> - <M> . <M>) / (3 eps_0 <V> k_B T),

with, per molecule type, the mean molecular dipole <|mu|>, <mu^2> and the finite-system Kirkwood factor
g_K = (<M_t^2> - <M_t>^2) / (N_t <mu^2>), the running eps_r against the number of frames used (does it converge?), and
the normalised autocorrelation Phi(t) of M, whose decay is the dielectric relaxation. The reference has no such module;
include/mdhip.h (mdhip_mol_moments) holds the specification of the device part, tests/dipole_ref.py restates both.

What runs where
  GPU (libmdhip.so, csrc/moments.hip): per batch of frames the raw dipole sum_k q_k (r_k - r_1) of every molecule (one
      wrap per atom against the molecule's first atom when the coordinates are wrapped) and, per type and frame, their
      sum and the sum of their squares, in a fixed order; Phi from `mdhip_xcorr`.
  Host: parsing (common/trajectory.py), the charges, the order of the frames, the averages and the CSV files.
"""

import os

import numpy as np
import pandas as pd

from .. import backend
from ..common import mol_series
from ..common import trajectory as T
from ..common.constants import BOLTZMANN, DIPOLE_CONVERSION, DISTANCE_CONVERSION, SUPPORTED_UNITS, VACUUM_PERMITTIVITY
from ..dist import is_writer

STREAM = True
BATCH_BYTES = None  # bytes of coordinates per streamed batch (None: the stream's own default)

NEUTRAL = 1.0e-6  # e: a type whose charges sum to more than this has an origin-dependent dipole and is left out of M
DEBYE = DIPOLE_CONVERSION["electron"]  # C m (the electron style's dipole unit is the debye)


def dielectric_from_series(total, sq_total, volume, n_mols, temperature, units="real"):
    """The averages behind calc_dielectric_constant from the per-type series, frames in time order: total [T,3,F] (the
    summed dipoles of the molecules of a type, in the dump's charge x distance units), sq_total [T,F] (the summed squares
    of the molecular dipoles), volume [F] (distance units cubed), n_mols [T]. Returns a dict:
      "M" [3,F] = the sum of the types in order; "eps_r"; "running" [F]: eps_r of the frames 0 .. n;
      "mu2" [T] = <mu^2>, "g_K" [T] = (<M_t . M_t> - <M_t> . <M_t>) / (N_t <mu^2>), both NaN for a type without
      molecules. Means are np.mean over the frames; a dot product is (x x + y y) + z z."""
    total, sq_total = np.asarray(total, dtype=np.float64), np.asarray(sq_total, dtype=np.float64)
    volume = np.asarray(volume, dtype=np.float64)
    n_types, _, F = total.shape
    M = np.zeros((3, F))
    for t in range(n_types):
        M = M + total[t]
    factor = DIPOLE_CONVERSION[units] ** 2 / (3.0 * VACUUM_PERMITTIVITY * DISTANCE_CONVERSION[units] ** 3 * BOLTZMANN
                                             * float(temperature))

    def fluctuation(m, upto):
        sq = (m[0, :upto] * m[0, :upto] + m[1, :upto] * m[1, :upto]) + m[2, :upto] * m[2, :upto]
        mean = [np.mean(m[x, :upto]) for x in range(3)]
        return np.mean(sq) - ((mean[0] * mean[0] + mean[1] * mean[1]) + mean[2] * mean[2])

    running = np.array([1.0 + factor * fluctuation(M, n) / np.mean(volume[:n]) for n in range(1, F + 1)])
    mu2 = np.full(n_types, np.nan)
    g_k = np.full(n_types, np.nan)
    for t in range(n_types):
        if n_mols[t]:
            mu2[t] = np.mean(sq_total[t]) / n_mols[t]
            with np.errstate(invalid="ignore", divide="ignore"):
                g_k[t] = fluctuation(total[t], F) / (n_mols[t] * mu2[t])
    return {"M": M, "eps_r": float(running[-1]), "running": running, "mu2": mu2, "g_K": g_k}


def calc_dielectric_constant(filename, num_mols, num_atoms_per_mol, temperature, units="real", mol_types=None,
                             coords="wrapped", dt=1, max_lag=None, save=False, working_dir=None):
    """
    The static dielectric constant of the frames of `filename` (dump file or '*' pattern; the `q` column is needed) at
    `temperature` (K), in the LAMMPS unit style `units`.
    num_mols / num_atoms_per_mol: molecules per type and atoms per molecule in id order; mol_types: the 1-based types
    whose dipoles make up M (default: all). Every molecule of a type must carry the same charges. A type whose charges
    do not sum to zero within 1e-6 e has a dipole that depends on the origin: it is left out of M and listed in
    `skipped` (its translation belongs to the conductivity, not to eps_r). coords="wrapped" reads `x y z` and wraps
    every atom once against the first atom of its molecule; coords="unwrapped" reads `xu yu zu` (or x y z ix iy iz).
    dt: timestep in fs, as `Reorientation`; max_lag: frames, None for no autocorrelation. Triclinic boxes are not
    supported.

    Returns a dict:
      "eps_r": 1 + (<M . M> - <M> . <M>) / (3 eps_0 <V> k_B T) over all frames;
      "types": DataFrame, one row per type in M: `mol_type`, `N`, `<|mu|> (D)` (the mean length of the molecular dipole
        in debye), `<mu^2> (D^2)`, `g_K` = (<M_t^2> - <M_t>^2) / (N <mu^2>), the finite-system Kirkwood factor;
      "convergence": DataFrame `frames`, `Time (ps)`, `eps_r`: the running value over the frames up to each one;
      "acf": with max_lag, DataFrame `Time (ps)`, `Phi` = sum over the axes of the autocorrelation of M - <M> at lag k,
        over the same at lag 0; else None;
      "skipped": the 1-based types left out because they carry a net charge.
    With `save`, dielectric_types.csv, dielectric_convergence.csv and dielectric_acf.csv go to working_dir (default: the
    current directory).
    """
    if coords not in ("wrapped", "unwrapped"):
        raise ValueError('coords must be "wrapped" or "unwrapped"')
    if units not in SUPPORTED_UNITS:
        raise ValueError("units must be one of %s" % ", ".join(SUPPORTED_UNITS))
    if not float(temperature) > 0.0:
        raise ValueError("temperature must be positive")
    num_mols, per = mol_series.layout(num_mols, num_atoms_per_mol)
    asked = list(range(1, len(per) + 1)) if mol_types is None else [int(t) for t in mol_types]
    if not asked or len(set(asked)) != len(asked) or not all(1 <= t <= len(per) for t in asked):
        raise ValueError("mol_types must be different types in [1, %d]" % len(per))
    from ..dynamical.conductivity import Conductivity

    T.refuse_triclinic(filename)
    wrapped = coords == "wrapped"

    def missing(lacking, _names):
        what = " (the dipoles need the charges)" if lacking[0] == "q" else ""
        raise ValueError(f"Missing column '{lacking[0]}' in dump file{what}.")

    _, batches = T.attribute_batches(filename, ("q", "type"), ["x", "y", "z"] if wrapped else T.UNWRAPPED,
                                     n_atoms=int(np.dot(num_mols, per)), with_box=True, stream=STREAM,
                                     batch_bytes=BATCH_BYTES, missing=missing)
    plan = None  # (kept types, skipped types, jobs, vector terms), once the first batch has shown the charges
    totals, squares, lengths, volumes, steps = [], [], [], [], []
    for ts, q, _types, xyz, box in batches:
        if plan is None:
            first = np.concatenate(([0], np.cumsum(np.multiply(num_mols, per))))
            rows = {t: mol_series.same_rows(q[0], int(first[t - 1]), num_mols[t - 1], per[t - 1], "charges",
                                            "%d:dipole" % t) for t in asked}
            skipped = [t for t in asked if abs(float(np.sum(rows[t]))) > NEUTRAL]
            kept = [t for t in asked if t not in skipped]
            if not kept:
                raise ValueError("every type of mol_types carries a net charge: there is no dipole to sum")
            plan = (kept, skipped, mol_series.type_jobs([t - 1 for t in kept], num_mols, per),
                    [[(k, float(rows[t][k])) for k in range(1, per[t - 1])] for t in kept])
        kept, skipped, (a0, mols, length), vec_terms = plan
        J = len(kept)
        got = backend.mol_moments(xyz, box if wrapped else None, a0, mols, length, [[] for _ in range(J)], vec_terms,
                                  np.zeros(J, dtype=np.int32), want_site=False, totals=True)
        vec = got["vec"]  # [B,3,S]: the lengths of the molecular dipoles, for <|mu|>
        norm = np.sqrt((vec[:, 0] * vec[:, 0] + vec[:, 1] * vec[:, 1]) + vec[:, 2] * vec[:, 2])
        off = np.concatenate(([0], np.cumsum(mols)))
        lengths.append(np.stack([norm[:, off[j]:off[j + 1]].sum(axis=1) for j in range(J)]))
        totals.append(got["total"])
        squares.append(got["sq_total"])
        box = np.asarray(box, dtype=np.float64)
        volumes.extend((box[:, 0] * box[:, 1] * box[:, 2]).tolist())
        steps.extend(np.asarray(ts).tolist())
    if plan is None:
        raise ValueError(f"no frames match {filename}")
    kept, skipped, (a0, mols, length), _ = plan
    order, times = Conductivity.frame_times(steps, dt * 10 ** -3)  # dt in fs -> ps per timestep unit, as Reorientation
    total = np.concatenate(totals, axis=2)[:, :, order]
    sq_total = np.concatenate(squares, axis=1)[:, order]
    abs_mu = np.concatenate(lengths, axis=1)[:, order]
    volume = np.asarray(volumes)[order]
    res = dielectric_from_series(total, sq_total, volume, mols, temperature, units)
    to_debye = DIPOLE_CONVERSION[units] / DEBYE
    with np.errstate(invalid="ignore", divide="ignore"):
        types_df = pd.DataFrame({"mol_type": kept, "N": [int(m) for m in mols],
                                 "<|mu|> (D)": [np.mean(abs_mu[j]) / mols[j] * to_debye if mols[j] else np.nan
                                                for j in range(len(kept))],
                                 "<mu^2> (D^2)": res["mu2"] * to_debye ** 2, "g_K": res["g_K"]})
    F = len(times)
    conv_df = pd.DataFrame({"frames": np.arange(1, F + 1), "Time (ps)": times - times[0], "eps_r": res["running"]})
    acf_df = None
    if max_lag is not None:
        max_lag = int(max_lag)
        if not 0 <= max_lag <= F - 1:
            raise ValueError("max_lag must be in [0, n_frames - 1 = %d]" % (F - 1))
        centred = np.ascontiguousarray(res["M"] - np.mean(res["M"], axis=1)[:, None])
        c = np.asarray(backend.xcorr(centred, n_lags=max_lag + 1)).reshape(3, max_lag + 1)
        s = (c[0] + c[1]) + c[2]
        with np.errstate(invalid="ignore", divide="ignore"):
            acf_df = pd.DataFrame({"Time (ps)": times[: max_lag + 1] - times[0], "Phi": s / s[0]})
    if save and is_writer():
        where = working_dir or os.getcwd()
        types_df.to_csv(where + "/dielectric_types.csv")
        conv_df.to_csv(where + "/dielectric_convergence.csv")
        if acf_df is not None:
            acf_df.to_csv(where + "/dielectric_acf.csv")
    return {"eps_r": res["eps_r"], "types": types_df, "convergence": conv_df, "acf": acf_df, "skipped": skipped}
