"""
Residence time of neighbours in a coordination shell — drop-in for
/root/reference/mdproptools/dynamical/residence_time.py (class `ResidenceTime`: residence_time.py:40-58,
70-146, 148-200; same constructor arguments, method names, defaults, files written).

What runs where
  GPU (libmdhip.so, `mdhip_shell_residence`): for every relation the shell indicator h_ij(t) of all
      (central atom, shell atom) pairs of every frame with the reference's exact single-wrap distance
      (residence_time.py:96-106) and the sum over pairs of the autocovariance numerators
      sum_t h_ij(t) h_ij(t+k) (residence_time.py:111-131) as exact integers.
  Host: parsing, the pseudo-type relabelling (`calc_atom_type`), normalisation (1/(n-k), 1/columns, /C(0)),
      the stretched-exponential fit (scipy.optimize.curve_fit, as upstream) and the CSV / PNG files.

Deliberate difference: with default ids (no num_mols / num_atoms_per_mol) the reference stops with a
broadcast ValueError (it hands `_calc_rsq(..., num_of_ids=0)` rows of [id, x, y, z]:
residence_time.py:96-101, rdf_cn.py:43); here that mode works and selects atoms by their LAMMPS type.

`Displacement` (residence_time.py:211-254): same constructor arguments and defaults, but the reference's `calc_dist`
is unfinished — it collects the wrapped x y z of the chosen atom types per frame, prints them and returns nothing; a
commented-out sketch groups the frames into windows of one residence time. Deliberate difference: here `calc_dist`
finishes that sketch — the distance every atom of a type travels over one residence time of its shell, over
consecutive (or all) time origins — and `calc_van_hove` gives the same distribution at any lags, G_s(r, t), with the
non-Gaussian parameter.
  GPU (`mdhip_displacement_hist`): image counts of the wrapped coordinates, the displacement of every (origin, atom)
      window, its histogram and the sums of r, r^2, r^4.
  Host: parsing, selection of the atoms by type, lag rounding, normalisation and the CSV files.
`calc_van_hove_distinct` adds the other half of the van Hove function, G_d(r, t): the density of atoms of type b at
time t0 + t at distance r from where an atom of type a was at t0, normalised like g(r) (at 0 ps it is g(r)).
  GPU (`mdhip_van_hove_distinct`): the pair histograms across the lag, all (pair, lag) jobs in one launch.
  Host: lag rounding, the ideal-gas normalisation and the CSV files.
"""

import math
import os

import numpy as np
import pandas as pd
from scipy.optimize import curve_fit
from scipy.special import gamma

from .. import backend
from ..common import sayer
from ..dist import is_writer
from ..common.com_mols import calc_atom_type
from ..common.trajectory import load_frames, load_typed_positions

VERBOSE = False


_say = sayer(globals())


class ResidenceTime:
    def __init__(self, r_cut, partial_relations, filename, dt=1, num_mols=None, num_atoms_per_mol=None,
                 working_dir=None):
        """
        r_cut: [lo, hi] per relation (a neighbour is counted when lo < r <= hi); partial_relations:
        [[central types...], [shell types...]]; filename: dump file or '*' pattern; dt: timestep in fs.
        """
        self.r_cut = r_cut
        self.relation_matrix = np.asarray(partial_relations).transpose()
        self.atom_pairs = []
        self.filename = filename
        self.dt = dt * 10 ** -3  # input dt in fs - convert to ps (residence_time.py:54)
        self.corr_df = None
        self.res_time_df = None
        self.num_mols = num_mols
        self.num_atoms_per_mol = num_atoms_per_mol
        self.working_dir = working_dir or os.getcwd()

    @staticmethod
    def _stretched_exp_function(x, a, tau_res, tau_short, beta):
        return a * np.exp(-((x / tau_res) ** beta)) + (1 - a) * np.exp(-x / tau_short)

    @staticmethod
    def _integrate_sum_exp(a, tau_res, tau_short, beta):
        return (a * tau_res * gamma(1 + 1 / beta)) + (1 - a) * tau_short

    def _labels(self, frame):
        """Type label of every (id-sorted) atom of one frame: LAMMPS type, or the index of the atom inside
        its molecule type when num_mols / num_atoms_per_mol are given (residence_time.py:85-93)."""
        if self.num_mols and self.num_atoms_per_mol:
            return calc_atom_type(frame.ids, self.num_mols, self.num_atoms_per_mol)
        return frame.types

    def calc_auto_correlation(self):
        frames = load_frames(self.filename)
        n = len(frames)
        correlation = {"Time (ps)": [fr.timestep * self.dt for fr in frames]}
        if n == 0:
            self.corr_df = pd.DataFrame.from_dict(correlation)
            return
        labels = self._labels(frames[0])
        for fr in frames[1:]:
            if fr.xyz.shape != frames[0].xyz.shape or not np.array_equal(self._labels(fr), labels):
                raise ValueError("every frame must hold the same atoms with the same types")
        xyz = np.stack([fr.xyz for fr in frames])  # [F,3,N], id-sorted
        box = np.asarray([fr.lengths for fr in frames], dtype=np.float64)
        lag_weight = (n - np.arange(n)).astype(np.float64)
        for kl in range(len(self.relation_matrix)):
            k, l = self.relation_matrix[kl]
            atom_pair = f"{k}-{l}"
            self.atom_pairs.extend([atom_pair] * n)  # the reference appends the label once per frame
            sel_k = np.flatnonzero(labels == k)
            sel_l = np.flatnonzero(labels == l)
            _say("relation", atom_pair, ":", len(sel_k), "central atoms,", len(sel_l), "shell atoms")
            xk = np.ascontiguousarray(xyz[:, :, sel_k])  # the library stages the two selections to the device
            xl = xk if k == l else np.ascontiguousarray(xyz[:, :, sel_l])
            counts, _ = backend.shell_residence(
                xk, xl, box, self.r_cut[kl][0] ** 2, self.r_cut[kl][1] ** 2, exclude_diagonal=bool(k == l))
            total_columns = float(len(sel_k) * len(sel_l))
            with np.errstate(invalid="ignore", divide="ignore"):
                corr = counts.astype(np.float64) / lag_weight / total_columns  # mean unbiased autocovariance
                corr = corr / corr[0]                                           # residence_time.py:142
            correlation[atom_pair] = corr
        self.corr_df = pd.DataFrame.from_dict(correlation)
        if is_writer():
            self.corr_df.to_csv(self.working_dir + "/auto_correlation.csv")

    def fit_auto_correlation(self, cut_percent=0.9, plot=True):
        residence_time = {}
        corr_data = self.corr_df.head(int(len(self.corr_df) * cut_percent))  # first part of the data
        for col in corr_data:
            if col == "Time (ps)":
                continue
            x = corr_data["Time (ps)"].values
            y = corr_data[col].values
            popt, _ = curve_fit(self._stretched_exp_function, x, y,
                                bounds=([0, 0, 0, 0.1], [np.inf, np.inf, np.inf, 1]), maxfev=5000)
            a, tau_res, tau_short, beta = popt
            residence_time[col] = [a, tau_res, tau_short, beta, self._integrate_sum_exp(a, tau_res, tau_short, beta)]
            if plot:
                self._plot_fit(corr_data, col, popt)
        print("Finished computing residence time")
        self.res_time_df = pd.DataFrame(residence_time)
        self.res_time_df.index = ["a", "tau_res", "tau_short", "beta", "r (ps)"]
        if is_writer():
            self.res_time_df.to_csv(self.working_dir + "/residence_time.csv")
        return residence_time

    def _plot_fit(self, corr_data, col, popt):
        import matplotlib

        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt

        from ..utilities.plots import set_axis

        fig, ax = plt.subplots(figsize=(8, 6))
        set_axis(ax)
        t = corr_data["Time (ps)"]
        ax.scatter(t, corr_data[col], color="red", label="original")
        ax.plot(t, self._stretched_exp_function(t.values, *popt), color="black", label="fit")
        ax.legend(frameon=False, fontsize=20)
        ax.set_xlabel("Time (ps)", fontsize=20)
        ax.set_ylabel("C(t)", fontsize=20)
        if is_writer():
            fig.savefig(self.working_dir + f"/{col}_fit.png", bbox_inches="tight", pad_inches=0.1)
        plt.close()


class Displacement:
    def __init__(self, atom_types, residence_time, filename, dt=1, save_mode=True, working_dir=None, bin_size=0.1,
                 r_max=None, overlap=False, coords="wrapped"):
        """
        atom_types: LAMMPS types to follow; residence_time: {type: time in ps} (the "r (ps)" row of
        ResidenceTime.fit_auto_correlation's table); filename: dump file or '*' pattern; dt: timestep in fs.
        bin_size, r_max: bins of the distance histograms, in the dump's length unit (r_max=None: half the smallest box
        edge of the trajectory); overlap: False = consecutive windows (origins one lag apart, the reference's
        pd.Grouper sketch), True = every frame is an origin.
        coords="wrapped" reads `id type x y z` as the reference does and rebuilds the periodic image counts on the
        GPU: only meaningful when no atom moves more than half a box edge between consecutive frames.
        coords="unwrapped" reads `xu yu zu`. Triclinic boxes are not supported. The dumps are read on first use.
        """
        if coords not in ("wrapped", "unwrapped"):
            raise ValueError('coords must be "wrapped" or "unwrapped"')
        self.atom_types = atom_types
        self.residence_time = residence_time
        self.filename = filename
        self.dt = dt * 10 ** -3  # input dt in fs (residence_time.py:224)
        self.save_mode = save_mode
        self.working_dir = working_dir or os.getcwd()
        self.bin_size = bin_size
        self.r_max = r_max
        self.overlap = overlap
        self.coords = coords
        self.dist_df = None
        self.hist_df = None
        self._traj = None

    def _load(self):
        """(r [F,3,E] the atoms of the requested types, grouped by type in the order of atom_types, ids ascending
        inside a type; box [F,3]; group_off [T+1]; frame spacing in ps)."""
        if self._traj is None:
            self._traj = load_typed_positions(self.filename, self.atom_types, self.coords, self.dt)
        return self._traj

    @staticmethod
    def _lag_frames(tau, delta):
        return max(1, int(math.floor(tau / delta + 0.5)))

    def _bins(self, box):
        r_max = 0.5 * float(box.min()) if self.r_max is None else float(self.r_max)
        return max(1, int(math.ceil(r_max / self.bin_size)))

    def _run(self, r, box, group_off, jobs, n_bins):
        return backend.displacement_hist(r, box if self.coords == "wrapped" else None, group_off, jobs,
                                         self.bin_size, n_bins)

    @staticmethod
    def _alpha2(moments, windows):
        with np.errstate(invalid="ignore", divide="ignore"):
            m2, m4 = moments[:, 1] / windows, moments[:, 2] / windows
            return 3.0 * m4 / (5.0 * (m2 * m2)) - 1.0

    def calc_dist(self):
        """Distance travelled by the atoms of every type during one residence time of that type: a row per type in
        `dist_df` (returned), the distance distributions (probability densities over r) in `hist_df`."""
        r, box, group_off, delta = self._load()
        n_frames = r.shape[0]
        lags = []
        for t in self.atom_types:
            k = self._lag_frames(self.residence_time[t], delta)
            if k > n_frames - 1:
                raise ValueError("the residence time of type %s (%g ps = %d frames) is longer than the trajectory "
                                 "(%d frames)" % (t, self.residence_time[t], k, n_frames))
            lags.append(k)
        jobs = [(g, k, 1 if self.overlap else k) for g, k in enumerate(lags)]
        n_bins = self._bins(box)
        hist, overflow, windows, moments, _ = self._run(r, box, group_off, jobs, n_bins)
        w = windows.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.dist_df = pd.DataFrame({
                "type": list(self.atom_types),
                "residence time (ps)": [self.residence_time[t] for t in self.atom_types],
                "lag (frames)": lags,
                "windows": windows.astype(np.int64),
                "mean distance": moments[:, 0] / w,
                "rms distance": np.sqrt(moments[:, 1] / w),
                "alpha2": self._alpha2(moments, w),
                "beyond r_max": overflow.astype(np.int64),
            })
            dist = {"r": (np.arange(n_bins) + 0.5) * self.bin_size}
            for g, t in enumerate(self.atom_types):
                dist[t] = hist[g] / (w[g] * self.bin_size)
        self.hist_df = pd.DataFrame(dist)
        if self.save_mode and is_writer():
            self.dist_df.to_csv(self.working_dir + "/displacement.csv")
            self.hist_df.to_csv(self.working_dir + "/displacement_distribution.csv")
        return self.dist_df

    def calc_van_hove(self, times):
        """Self part of the van Hove function at the lags `times` (ps; rounded to frames, duplicates dropped), every
        frame an origin: ({type: DataFrame of r and G_s(r, t) per lag time as a probability density over r},
        DataFrame of the non-Gaussian parameter alpha2 = 3 <r^4> / (5 <r^2>^2) - 1 per lag time and type)."""
        r, box, group_off, delta = self._load()
        n_frames = r.shape[0]
        lags = []
        for t in times:
            k = self._lag_frames(t, delta)
            if k > n_frames - 1:
                raise ValueError("the time %g ps (%d frames) is longer than the trajectory (%d frames)"
                                 % (t, k, n_frames))
            if k not in lags:
                lags.append(k)
        lag_ps = [k * delta for k in lags]
        jobs = [(g, k, 1) for g in range(len(self.atom_types)) for k in lags]
        n_bins = self._bins(box)
        hist, _, windows, moments, _ = self._run(r, box, group_off, jobs, n_bins)
        w = windows.astype(np.float64)
        a2 = self._alpha2(moments, w)
        gs, alpha2 = {}, {"Time (ps)": lag_ps}
        n = len(lags)
        for g, t in enumerate(self.atom_types):
            cols = {"r": (np.arange(n_bins) + 0.5) * self.bin_size}
            with np.errstate(invalid="ignore", divide="ignore"):
                for i, tp in enumerate(lag_ps):
                    cols[tp] = hist[g * n + i] / (w[g * n + i] * self.bin_size)
            gs[t] = pd.DataFrame(cols)
            alpha2[t] = a2[g * n:(g + 1) * n]
        alpha2 = pd.DataFrame(alpha2)
        if self.save_mode and is_writer():
            for t, df in gs.items():
                df.to_csv(self.working_dir + "/van_hove_%s.csv" % t)
            alpha2.to_csv(self.working_dir + "/alpha2.csv")
        return gs, alpha2

    def calc_van_hove_distinct(self, times, pairs=None, origin_stride=1):
        """Distinct part of the van Hove function at the lags `times` (ps; rounded to frames, 0 ps is lag 0, duplicates
        dropped), every `origin_stride`-th frame an origin: ({(type a, type b): DataFrame of r and G_d(r, t) per lag
        time}, DataFrame of `pairs` and `beyond r_max` per (pair, lag)). G_d = hist / ((origins N_a) rho_b shell) with
        rho_b = N_b / mean volume of the origin frames and shell = 4/3 pi bin_size^3 ((bin+1)^3 - bin^3): the g(r)
        normalisation, so the 0 ps column is g_a-b(r). `pairs`: (type a, type b) tuples, both from atom_types; default
        every unordered pair, same-type pairs included."""
        if self.coords != "wrapped":
            raise ValueError('calc_van_hove_distinct needs coords="wrapped": the single periodic wrap between two atoms '
                             "is taken on the wrapped x y z")
        if int(origin_stride) < 1:
            raise ValueError("origin_stride must be at least 1")
        stride = int(origin_stride)
        r, box, group_off, delta = self._load()
        n_frames = r.shape[0]
        lags = []
        for t in times:
            k = int(math.floor(t / delta + 0.5))
            if k < 0:
                raise ValueError("the time %g ps is negative" % t)
            if k > n_frames - 1:
                raise ValueError("the time %g ps (%d frames) is longer than the trajectory (%d frames)"
                                 % (t, k, n_frames))
            if k not in lags:
                lags.append(k)
        types = list(self.atom_types)
        if pairs is None:
            pairs = [(a, b) for i, a in enumerate(types) for b in types[i:]]
        pairs = [tuple(p) for p in pairs]
        for a, b in pairs:
            if a not in types or b not in types:
                raise ValueError("pair (%s, %s): both types must be in atom_types" % (a, b))
        jobs = [(types.index(a), types.index(b), k, stride) for a, b in pairs for k in lags]
        n_bins = self._bins(box)
        hist, beyond, n_pairs = backend.van_hove_distinct(r, box, group_off, jobs, self.bin_size, n_bins)
        k_bin = np.arange(n_bins, dtype=np.float64)
        shell = 4.0 / 3.0 * math.pi * self.bin_size ** 3 * ((k_bin + 1.0) ** 3 - k_bin ** 3)
        volume = box[:, 0] * box[:, 1] * box[:, 2]
        sizes = np.diff(group_off)
        gd, summary = {}, {"pair": [], "Time (ps)": [], "origins": [], "pairs": [], "beyond r_max": []}
        for p, (a, b) in enumerate(pairs):
            n_a, n_b = float(sizes[types.index(a)]), float(sizes[types.index(b)])
            cols = {"r": (k_bin + 0.5) * self.bin_size}
            for i, k in enumerate(lags):
                j = p * len(lags) + i
                origins = np.arange(0, n_frames - k, stride)
                rho_b = n_b / np.mean(volume[origins])
                with np.errstate(invalid="ignore", divide="ignore"):
                    cols[k * delta] = hist[j] / ((len(origins) * n_a) * rho_b * shell)
                summary["pair"].append("%s-%s" % (a, b))
                summary["Time (ps)"].append(k * delta)
                summary["origins"].append(len(origins))
                summary["pairs"].append(int(n_pairs[j]))
                summary["beyond r_max"].append(int(beyond[j]))
            gd[(a, b)] = pd.DataFrame(cols)
        summary = pd.DataFrame(summary)
        if self.save_mode and is_writer():
            for (a, b), df in gd.items():
                df.to_csv(self.working_dir + "/van_hove_distinct_%s-%s.csv" % (a, b))
            summary.to_csv(self.working_dir + "/van_hove_distinct_pairs.csv")
        return gd, summary
