"""
Molecular reorientation: the first- and second-rank orientational time-correlation functions of molecule-fixed unit
vectors,

    C_l(k) = < P_l( u_m(t) . u_m(t + k) ) >   over the molecules m of a type and the time origins t,   l = 1, 2,

and the relaxation times read from them. The reference has no such module; the constructor follows `Displacement`
(dynamical/residence_time.py) and the molecule layout arguments follow `Conductivity`.

What runs where
  GPU (libmdhip.so): `mdhip_axis_vectors` reduces every batch of frames to the unit vectors U [S,3,F] (a bond or
      end-to-end vector tail -> head, or the dipole about the molecule's first atom; wrapped coordinates are put
      together again by one wrap per atom against the first atom of the molecule), which stay on the device;
      `mdhip_orient_corr` sums u(t) . u(t+k) and its square over molecules and origins at every lag; the running
      integral of the relaxation times is `mdhip_cumtrapz`.
  Host: parsing (common/trajectory.py: the frames are never all resident), the order and spacing of the frames,
      C1 = S1 / W, C2 = 1.5 S2 / W - 0.5, the log-linear fit and the CSV / PNG files.
"""

import math
import os

import numpy as np
import pandas as pd

from .. import backend
from ..common import mol_series
from ..common.trajectory import refuse_triclinic
from ..dist import is_writer

# True: the dumps are parsed into page-locked staging batches and each is reduced on the GPU while the next one is
# being parsed (mdproptools_amd/stream.py). False: every frame is parsed first and reduced in one call.
STREAM = True
BATCH_BYTES = None  # bytes of coordinates per streamed batch (None: the stream's own default)

MAX_VECTORS = backend.ORIENT_MAX_GROUPS


def _label(vec):
    return "%d:dipole" % vec[0] if vec[1] == "dipole" else "%d:%d-%d" % vec


class Reorientation:
    def __init__(self, vectors, filename, num_mols, num_atoms_per_mol, dt=1, working_dir=None, coords="wrapped"):
        """
        vectors: list of (mol_type, tail, head) — mol_type the 1-based index into num_mols, tail and head 1-based
        indices of atoms inside the molecule: the vector points from tail to head — or (mol_type, "dipole"): the
        dipole moment sum_k q_k (r_k - r_1) about the molecule's first atom (the dump's `q` column; for a charged
        molecule the dipole depends on that origin). Several vectors may name one molecule type; at most 16.
        filename: dump file or '*' pattern; num_mols / num_atoms_per_mol: molecules per type and atoms per molecule in
        id order; dt: timestep in fs, as in `Displacement` (`self.dt` keeps it in ps per timestep unit); working_dir:
        where the CSV files go (default: the current directory; `self.save_mode = False` writes none).
        coords="wrapped" reads `x y z` and the box: every named atom is wrapped once against the first atom of its
        molecule, which is only meaningful when the named atoms lie within half a box edge of it. coords="unwrapped"
        reads `xu yu zu` (or builds them from x y z ix iy iz). Triclinic boxes are not supported. The dumps are read on
        first use.
        """
        if coords not in ("wrapped", "unwrapped"):
            raise ValueError('coords must be "wrapped" or "unwrapped"')
        self.num_mols, self.num_atoms_per_mol = mol_series.layout(num_mols, num_atoms_per_mol)
        self.vectors = self._checked(vectors, self.num_atoms_per_mol)
        self.labels = [_label(v) for v in self.vectors]
        self.filename = filename
        self.dt = dt * 10 ** -3  # input dt in fs, as Displacement
        self.save_mode = True
        self.working_dir = working_dir or os.getcwd()
        self.coords = coords
        self.corr_df = None
        self.relax_df = None
        self.degenerate = None
        self._traj = None

    @staticmethod
    def _checked(vectors, atoms_per_mol):
        vectors = list(vectors)
        if not vectors:
            raise ValueError("vectors must name at least one (mol_type, tail, head) or (mol_type, 'dipole')")
        if len(vectors) > MAX_VECTORS:
            raise ValueError("at most %d vectors per instance (%d given)" % (MAX_VECTORS, len(vectors)))
        out = []
        for v in vectors:
            v = tuple(v)
            dipole = len(v) == 2 and v[1] == "dipole"
            if not dipole and len(v) != 3:
                raise ValueError("a vector is (mol_type, tail, head) or (mol_type, 'dipole'): %r" % (v,))
            mol_type = int(v[0])
            if not 1 <= mol_type <= len(atoms_per_mol):
                raise ValueError("vector %r: mol_type must be in [1, %d]" % (v, len(atoms_per_mol)))
            n = atoms_per_mol[mol_type - 1]
            if dipole:
                if n < 2:
                    raise ValueError("vector %r: a dipole needs a molecule of at least two atoms" % (v,))
                out.append((mol_type, "dipole"))
                continue
            tail, head = int(v[1]), int(v[2])
            if not (1 <= tail <= n and 1 <= head <= n):
                raise ValueError("vector %r: tail and head must be in [1, %d], the atoms of a molecule of type %d"
                                 % (v, n, mol_type))
            if tail == head:
                raise ValueError("vector %r: tail and head are the same atom" % (v,))
            out.append((mol_type, tail, head))
        return out

    # ---- the unit vectors ---------------------------------------------------------------------------------------------

    def _jobs(self):
        """(job_atom0, job_mols, job_len) of the vectors: one job per vector, over all molecules of its type."""
        return mol_series.type_jobs([v[0] - 1 for v in self.vectors], self.num_mols, self.num_atoms_per_mol)

    def _terms(self, q):
        """Per vector the terms [(k, w)], k ascending from 1: (tail, -1), (head, +1) without the first atom's, or the
        charges q_k of the atoms of the type's first molecule (every molecule of the type must carry the same)."""
        a0, mols, length = self._jobs()
        terms = []
        for v, start, m, n in zip(self.vectors, a0, mols, length):
            if v[1] == "dipole":
                qm = np.asarray(q[start:start + m * n], dtype=np.float64).reshape(m, n)
                if m and np.any(qm != qm[0]):
                    raise ValueError("vector %s: the molecules of type %d do not all carry the same charges"
                                     % (_label(v), v[0]))
                terms.append([(k, float(qm[0, k]) if m else 0.0) for k in range(1, n)])
            else:
                pair = [(v[1] - 1, -1.0), (v[2] - 1, 1.0)]
                terms.append(sorted(t for t in pair if t[0] > 0))
        return terms

    def _refuse_degenerate(self, degenerate):
        """Keeps the zero-vector counts of the vectors; a direction that does not exist has no correlation function."""
        self.degenerate = np.asarray(degenerate, dtype=np.uint64)
        mol_series.refuse_degenerate(self.labels, self.degenerate, "zero-length vectors",
                                     "Tail and head coincide there, or the dipole vanishes")

    def _load(self):
        """(U [S,3,F] float64 CUDA tensor, frames in time order; times [F] in ps; group_off [V+1]): read once."""
        if self._traj is not None:
            return self._traj
        refuse_triclinic(self.filename)
        dipole = any(v[1] == "dipole" for v in self.vectors)
        a0, mols, length = self._jobs()

        def missing(lacking, _names):
            what = " (a dipole needs the charges)" if lacking[0] == "q" else ""
            raise ValueError(f"Missing column '{lacking[0]}' in dump file{what}.")

        terms = []  # of every vector, once the first batch has shown the charges

        def compute(xyz, box, out, ctx, first):
            if not terms:
                terms.extend(self._terms(first[0] if dipole else None))
            return backend.axis_vectors(xyz, box, a0, mols, length, terms, out=out, ctx=ctx)[1]

        V = len(self.vectors)
        U, times, group_off, degenerate = mol_series.load_series(
            self.filename, self.coords, int(np.dot(self.num_mols, self.num_atoms_per_mol)), compute, mols, np.arange(V), V,
            self.dt, lead="q" if dipole else "id", stream=STREAM, batch_bytes=BATCH_BYTES, missing=missing)
        self._refuse_degenerate(degenerate)
        self._traj = (U, times, group_off)
        return self._traj

    # ---- correlation functions ----------------------------------------------------------------------------------------

    def calc_correlation(self, max_lag=None, plot=False):
        """C1 and C2 of every vector at the lags 0 .. max_lag frames (default (F - 1) // 2): a DataFrame `Time (ps)`,
        `C1_<label>`, `C2_<label>` per vector, label = `type:tail-head` or `type:dipole`; kept in `self.corr_df` and,
        with save_mode, written to reorientation.csv (plot: reorientation.png) in working_dir."""
        U, times, group_off = self._load()
        max_lag, sums = mol_series.orient_corr(U, group_off, max_lag)
        cols = {"Time (ps)": times[: max_lag + 1] - times[0]}
        origins = (len(times) - np.arange(max_lag + 1)).astype(np.float64)
        for g, lab in enumerate(self.labels):
            w = origins * float(group_off[g + 1] - group_off[g])
            with np.errstate(invalid="ignore", divide="ignore"):
                cols["C1_" + lab] = sums[:, g, 0] / w
                cols["C2_" + lab] = 1.5 * sums[:, g, 1] / w - 0.5
        self.corr_df = pd.DataFrame(cols)
        if self.save_mode and is_writer():
            self.corr_df.to_csv(self.working_dir + "/reorientation.csv")
        if plot and is_writer():
            self._plot_correlation()
        return self.corr_df

    def calc_relaxation_times(self, t_cut=None, fit_floor=math.exp(-2)):
        """One row per vector and rank l = 1, 2 (computes the correlation functions with their defaults when there are
        none yet):
          tau_integral (ps): the trapezoid integral of C_l from 0 to t_cut (default: the first lag at which C_l <= 0,
            else the last lag; a given t_cut is rounded down to a lag);
          tau_fit (ps), amplitude: C_l ~ amplitude * exp(-t / tau_fit), from the ordinary least-squares line through
            ln C_l over the leading run of lags with C_l >= fit_floor (fit_lags of them); NaN with fewer than two.
        Kept in `self.relax_df`; with save_mode written to reorientation_times.csv."""
        if self.corr_df is None:
            self.calc_correlation()
        t = self.corr_df["Time (ps)"].to_numpy(dtype=np.float64)
        names = [c for c in self.corr_df.columns if c != "Time (ps)"]
        Y = np.ascontiguousarray(self.corr_df[names].to_numpy(dtype=np.float64).T)
        n = len(t)
        dx = float(t[1] - t[0]) if n > 1 else 1.0
        running = np.asarray(backend.cumtrapz(Y, dx, leading_zero=True)).reshape(len(names), n) if n > 1 else \
            np.zeros((len(names), n))
        rows = []
        for s, name in enumerate(names):
            c = Y[s]
            if t_cut is None:
                below = np.flatnonzero(c <= 0.0)
                i_cut = int(below[0]) if len(below) else n - 1
            else:
                i_cut = int(np.clip(np.searchsorted(t, float(t_cut), side="right") - 1, 0, n - 1))
            ok = c >= fit_floor  # (False for a NaN)
            run = n if ok.all() else int(np.argmin(ok))
            tau_fit = amplitude = float("nan")
            if run >= 2:
                tc = t[:run] - t[:run].mean()
                y = np.log(c[:run])
                with np.errstate(divide="ignore"):
                    slope = float(np.dot(tc, y - y.mean()) / np.dot(tc, tc))
                    tau_fit = -1.0 / slope
                amplitude = float(math.exp(y.mean() - slope * t[:run].mean()))
            rank, label = name[1], name[3:]
            rows.append({"vector": label, "rank": int(rank), "t_cut (ps)": float(t[i_cut]),
                         "tau_integral (ps)": float(running[s, i_cut]), "tau_fit (ps)": tau_fit,
                         "amplitude": amplitude, "fit_lags": run})
        self.relax_df = pd.DataFrame(rows)
        if self.save_mode and is_writer():
            self.relax_df.to_csv(self.working_dir + "/reorientation_times.csv")
        return self.relax_df

    def _plot_correlation(self):
        import matplotlib

        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt

        from ..utilities.plots import set_axis

        t = self.corr_df["Time (ps)"].to_numpy()
        cmap = plt.get_cmap("Paired")
        fig, ax = plt.subplots(1, 1, figsize=(10, 5))
        for i, lab in enumerate(self.labels):
            ax.plot(t, self.corr_df["C1_" + lab], linewidth=2, color=cmap((2 * i + 1) / 12), label=r"$C_1$ " + lab)
            ax.plot(t, self.corr_df["C2_" + lab], linewidth=2, color=cmap((2 * i) / 12), label=r"$C_2$ " + lab)
        ax.axhline(0.0, linewidth=1, color="black", linestyle="--")
        set_axis(ax, axis="both")
        ax.set_xlabel(r"$\mathrm{Time, ps}$", fontsize=18)
        ax.set_ylabel(r"$\mathrm{C_l(t)}$", fontsize=18)
        ax.legend(fontsize=16, loc="center left", bbox_to_anchor=(1, 0.5), frameon=False)
        fig.tight_layout(pad=3)
        fig.savefig(f"{self.working_dir}/reorientation.png", bbox_inches="tight", pad_inches=0.1)
        plt.close(fig)
