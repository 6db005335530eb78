"""
Structural relaxation of the atoms of chosen types — no counterpart in the reference, which stops at the MSD and the
residence time. The two quantities computed right after the MSD of a viscous electrolyte or ionic liquid:

  F_s(q, t) = < sin(q |dr|) / (q |dr|) >            the self-intermediate scattering function, isotropic and exact;
                                                    its 1/e time is the structural (alpha) relaxation time
  Q(t)      = < theta(a - |dr|) >                   the overlap function
  chi4(t)   = N [ <Q^2> - <Q>^2 ] over time origins the four-point susceptibility; its peak gives the time and the
                                                    strength of dynamic heterogeneity

dr = r(t0 + t) - r(t0) of one atom, the averages over the atoms of a type and the time origins t0.

What runs where
  GPU (`mdhip_self_relaxation`): the image counts of wrapped coordinates, and for every lag and time origin the
      number n(t0, k) of atoms within `a` of where they were, its sums n and n^2 over origins, and the sum of
      sinc(q |dr|) as an exact 2^32 fixed-point integer.
  Host: parsing (the loader of `Displacement`), selection of the atoms by type, normalisation — chi4's numerator in
      exact Python integers, since a float64 difference of two numbers near 2^80 cancels — the crossing times and the
      CSV files. Under torch.distributed every rank computes and only the writer writes, as `Reorientation` does.
"""

import os

import numpy as np
import pandas as pd

from .. import backend
from ..common.trajectory import load_typed_positions
from ..dist import is_writer

MAX_TYPES = backend.RELAX_MAX_GROUPS
MAX_Q = backend.RELAX_MAX_Q
FS_UNIT = 1 << 32


def chi4_exact(origins, count1, count2, n):
    """(O count2 - count1^2) / (O^2 N) per lag, the numerator in exact integers; 0 where O <= 1 or N = 0."""
    out = np.zeros(len(origins))
    for k, (o, c1, c2) in enumerate(zip(origins, count1, count2)):
        o, c1, c2 = int(o), int(c1), int(c2)
        if o > 1 and n > 0:
            num = o * c2 - c1 * c1
            den = o * o * int(n)
            out[k] = num / den  # (Python's true division of integers is correctly rounded)
    return out


def first_crossing(t, y, level):
    """The time at which y first falls below `level`, linearly interpolated between the two lags; NaN if it never
    does (or is not above it at the start)."""
    y = np.asarray(y, dtype=np.float64)
    below = np.flatnonzero(y < level)
    if len(below) == 0:
        return float("nan")
    i = int(below[0])
    if i == 0:
        return float(t[0])
    y0, y1 = float(y[i - 1]), float(y[i])
    return float(t[i - 1] + (t[i] - t[i - 1]) * (y0 - level) / (y0 - y1))


class StructuralRelaxation:
    def __init__(self, atom_types, filename, dt=1, save_mode=True, working_dir=None, coords="wrapped"):
        """
        atom_types: LAMMPS types to follow (at most 16); filename: dump file or '*' pattern; dt: timestep in fs.
        coords="wrapped" reads `id type x y z` and rebuilds the periodic image counts on the GPU: only meaningful when
        no atom moves more than half a box edge between consecutive frames. coords="unwrapped" reads `xu yu zu`.
        Triclinic boxes are not supported; the frames must be uniformly spaced. The dumps are read on first use.
        """
        if coords not in ("wrapped", "unwrapped"):
            raise ValueError('coords must be "wrapped" or "unwrapped"')
        atom_types = list(atom_types)
        if not 1 <= len(atom_types) <= MAX_TYPES:
            raise ValueError("atom_types must name 1 to %d types" % MAX_TYPES)
        self.atom_types = atom_types
        self.filename = filename
        self.dt = dt * 10 ** -3  # input dt in fs, as Displacement
        self.save_mode = save_mode
        self.working_dir = working_dir or os.getcwd()
        self.coords = coords
        self.relax_df = None
        self.times_df = None
        self._traj = None
        self._q = None

    def _load(self):
        if self._traj is None:
            self._traj = load_typed_positions(self.filename, self.atom_types, self.coords, self.dt,
                                              what="a relaxation function")
        return self._traj

    def _per_type(self, value, name, many):
        """`value` (a number, a list when `many`, or {type: either}) as one list per type."""
        rows = []
        for t in self.atom_types:
            if isinstance(value, dict):
                if t not in value:
                    raise ValueError("%s has no entry for type %s" % (name, t))
                v = value[t]
            else:
                v = value
            v = [float(x) for x in np.atleast_1d(np.asarray(v, dtype=np.float64))]
            if not many and len(v) != 1:
                raise ValueError("%s takes one number per type" % name)
            rows.append(v)
        if len({len(v) for v in rows}) != 1:
            raise ValueError("%s must hold the same number of values for every type" % name)
        return rows

    def calc_relaxation(self, q=None, a=None, max_lag=None, origin_stride=1, plot=False):
        """F_s(q, t), Q(t) and chi4(t) of every type at the lags 0 .. max_lag frames (default (F - 1) // 2), every
        `origin_stride`-th frame an origin. q: a wave number (1 / length unit of the dump), a list of up to 4, or
        {type: number | list}; a: the overlap length, a number or {type: number}; at least one of the two.
        Returns a DataFrame `Time (ps)`, `origins` and per type `Fs_<type>_q<value>`, `Q_<type>`, `chi4_<type>`; kept
        in `self.relax_df` and, with save_mode, written to relaxation.csv (plot: relaxation.png) in working_dir."""
        if q is None and a is None:
            raise ValueError("at least one of q and a must be given")
        qs = None if q is None else self._per_type(q, "q", True)
        if qs is not None and not 1 <= len(qs[0]) <= MAX_Q:
            raise ValueError("q must hold 1 to %d wave numbers per type" % MAX_Q)
        for t, row in zip(self.atom_types, qs or []):
            names = ["%g" % v for v in row]
            if len(set(names)) != len(names):  # (two columns of one name would overwrite each other)
                raise ValueError("type %s: the wave numbers %s give the column names %s: they must differ in six "
                                 "significant digits" % (t, row, names))
        av = None if a is None else [v[0] for v in self._per_type(a, "a", False)]
        r, box, group_off, delta = self._load()
        n_frames = r.shape[0]
        if max_lag is None:
            max_lag = (n_frames - 1) // 2
        max_lag = int(max_lag)
        if not 0 <= max_lag <= n_frames - 1:
            raise ValueError("max_lag must be in [0, n_frames - 1 = %d]" % (n_frames - 1))
        origins, count1, count2, fs, nonfinite = backend.self_relaxation(
            r, box if self.coords == "wrapped" else None, group_off, max_lag, origin_stride=int(origin_stride), a=av,
            q=qs)
        cols = {"Time (ps)": np.arange(max_lag + 1) * delta, "origins": origins.astype(np.int64)}
        o = origins.astype(np.float64)
        for g, t in enumerate(self.atom_types):
            bad = np.flatnonzero(nonfinite[:, g])
            if len(bad):
                raise ValueError("type %s: %d displacements at lag %d (the first of %d lags) are not finite: the "
                                 "trajectory holds NaN or Inf coordinates" % (t, int(nonfinite[bad[0], g]), int(bad[0]),
                                                                              len(bad)))
            n = int(group_off[g + 1] - group_off[g])
            with np.errstate(invalid="ignore", divide="ignore"):
                w = o * float(n)
                if qs is not None:
                    for j, qj in enumerate(qs[g]):
                        cols["Fs_%s_q%g" % (t, qj)] = fs[:, g, j].astype(np.float64) / float(FS_UNIT) / w
                if av is not None:
                    cols["Q_%s" % t] = count1[:, g].astype(np.float64) / w
                    cols["chi4_%s" % t] = chi4_exact(origins, count1[:, g], count2[:, g], n)
        self._q = qs
        self.relax_df = pd.DataFrame(cols)
        if self.save_mode and is_writer():
            self.relax_df.to_csv(self.working_dir + "/relaxation.csv")
        if plot and is_writer():
            self._plot()
        return self.relax_df

    def calc_relaxation_times(self):
        """One row per (type, q) — `tau_alpha (ps)`: the first crossing of F_s below 1/e, linearly interpolated between
        the two lags, NaN if F_s never crosses — and one row per type — `tau_Q (ps)`: the same for Q; `t_star (ps)`,
        `chi4_max`: the lag of the largest chi4 and its value. Needs calc_relaxation first. Kept in `self.times_df`;
        with save_mode written to relaxation_times.csv."""
        if self.relax_df is None:
            raise ValueError("calc_relaxation has to run first")
        df = self.relax_df
        t = df["Time (ps)"].to_numpy(dtype=np.float64)
        level = float(np.exp(-1.0))
        nan = float("nan")
        rows = []
        for g, typ in enumerate(self.atom_types):
            for qj in (self._q[g] if self._q is not None else []):
                rows.append({"type": typ, "q": qj, "tau_alpha (ps)": first_crossing(t, df["Fs_%s_q%g" % (typ, qj)], level),
                             "tau_Q (ps)": nan, "t_star (ps)": nan, "chi4_max": nan})
            if "Q_%s" % typ in df:
                chi4 = df["chi4_%s" % typ].to_numpy(dtype=np.float64)
                peak = int(np.nanargmax(chi4)) if np.isfinite(chi4).any() else 0
                rows.append({"type": typ, "q": nan, "tau_alpha (ps)": nan,
                             "tau_Q (ps)": first_crossing(t, df["Q_%s" % typ], level), "t_star (ps)": float(t[peak]),
                             "chi4_max": float(chi4[peak])})
        self.times_df = pd.DataFrame(rows, columns=["type", "q", "tau_alpha (ps)", "tau_Q (ps)", "t_star (ps)",
                                                    "chi4_max"])
        if self.save_mode and is_writer():
            self.times_df.to_csv(self.working_dir + "/relaxation_times.csv")
        return self.times_df

    def _plot(self):
        import matplotlib

        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt

        from ..utilities.plots import set_axis

        t = self.relax_df["Time (ps)"].to_numpy()
        fig, axes = plt.subplots(1, 2, figsize=(14, 5))
        for c in self.relax_df.columns:
            if c.startswith(("Fs_", "Q_")):
                axes[0].plot(t[1:], self.relax_df[c][1:], linewidth=2, label=c)
            elif c.startswith("chi4_"):
                axes[1].plot(t[1:], self.relax_df[c][1:], linewidth=2, label=c)
        axes[0].axhline(float(np.exp(-1.0)), linewidth=1, color="black", linestyle="--")
        for ax, label in zip(axes, (r"$F_s(q,t),\ Q(t)$", r"$\chi_4(t)$")):
            set_axis(ax, axis="both")
            ax.set_xscale("log")
            ax.set_xlabel(r"$\mathrm{Time, ps}$", fontsize=18)
            ax.set_ylabel(label, fontsize=18)
            ax.legend(fontsize=12, frameon=False)
        fig.tight_layout(pad=3)
        fig.savefig(f"{self.working_dir}/relaxation.png", bbox_inches="tight", pad_inches=0.1)
        plt.close(fig)
