"""
Green-Kubo ionic conductivity from LAMMPS dumps — drop-in for
/root/reference/mdproptools/dynamical/conductivity.py (class `Conductivity`, same method names,
argument order, defaults and files written: conductivity.py:51-62, 98, 117, 167, 197, 216, 234, 259, 276).

What runs where
  GPU (libmdhip.so): the per-frame molecular charge flux for ALL frames in one call
      (`conductivity_loop`, _conductivity.py:7-36 — the step the reference marks as its slowest and
      spreads over a process pool), every flux cross-correlation (conductivity.py:97-114, batched)
      and the running integrals (conductivity.py:216-232).
  Host: parsing, plateau detection (pandas, conductivity.py:116-165), the final Green-Kubo factor.

`einstein` and `nernst` (`pass` in the reference, conductivity.py:399-403) are the Einstein-Helfand route to the same
numbers, from positions instead of velocities: molecule centres of mass (mdhip_segment_com), their charge-weighted
collective displacement per molecule type (mdhip_collective_displacement), its cross-displacement correlation at every
lag (mdhip_cross_msd; the self part through mdhip_lag_msd) on the GPU; the straight-line fit and the 1 / (6 kB T V)
factor on the host. `ionicity` is their ratio.
"""

import glob
import os

import numpy as np
import pandas as pd

from .. import backend
from ..common import constants
from ..common import trajectory as T
from ..common.com_mols import molecule_layout
from ..io import parse_lammps_dumps

# True: get_charge_flux parses into page-locked staging batches and runs the fused flux kernel on each while the next
# one is being parsed (mdproptools_amd/stream.py). False: every frame is parsed first (round-1 route).
STREAM = True


class Conductivity:
    """Green-Kubo ionic conductivity (total and per molecule type) following 10.1063/1.4890741."""

    def __init__(self, filename, num_mols, num_atoms_per_mol, volume, mass=None, temp=298.15, timestep=1,
                 units="real", working_dir=None):
        """
        filename: dump file pattern; num_mols / num_atoms_per_mol: molecules per type and atoms per
        molecule in dump order; volume: box volume in `units`; mass: per-atom-type masses (or None to
        read the dump's mass column); temp [K]; timestep in `units`; working_dir: where the dumps are.
        """
        self.working_dir = working_dir or os.getcwd()
        self.filename = filename
        self.dumps = parse_lammps_dumps(f"{self.working_dir}/{self.filename}")
        self.mass = mass
        self.num_mols = num_mols
        self.num_atoms_per_mol = num_atoms_per_mol
        self.units = units
        self.volume = volume * constants.DISTANCE_CONVERSION[self.units] ** 3  # m^3
        self.temp = temp
        self.timestep = timestep
        self.time = []  # seconds, one entry per frame, filled by get_charge_flux

    @staticmethod
    def correlate(a, b):
        """c[k] = sum_t a[t+k] b[t] / (n-k), evaluated with zero-padded FFTs on the GPU."""
        return backend.xcorr(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64),
                             method=backend.XCORR_FFT)

    @staticmethod
    def detect_time_range(flux, tol):
        """
        (start, end) indices of the longest stretch where the correlation function is flat: the series
        is cut into blocks, the block standard deviations are scaled by their own spread, compared
        with `tol`, smoothed with a centred rolling median and the longest run of ones is returned
        (conductivity.py:116-165).
        """
        flux = pd.Series(flux, name="flux")
        block = max(int(len(flux) / 10000), 5)
        labels = np.arange(len(flux)) // block
        block_std = flux.groupby(labels).transform("std")
        spread = block_std.std()
        flat = ((block_std / (spread if spread else 1)) < tol).astype("int").to_frame()
        smooth = (flat.rolling(window=4 * block + 1, min_periods=3 * block + 1, center=True)
                  .median().fillna(0)["flux"].to_numpy())
        on = smooth == 1
        runs, start = [], None
        for k in range(len(smooth)):
            if on[k] and start is None:
                start = k
            elif smooth[k] < 1 and start is not None:
                runs.append((start, k))
                start = None
        if start is not None:
            runs.append((start, len(smooth) - 1))
        best, best_len = None, 0
        for run in runs:
            if run[1] - run[0] > best_len:
                best, best_len = run, run[1] - run[0]
        if best is None:
            raise TypeError("list indices must be integers or slices, not NoneType")  # as the reference
        return best

    def get_charge_flux(self):
        """Charge flux J[3, n_types, n_frames] in SI units; also fills `self.time` (conductivity.py:167-195)."""
        from .. import dist as D
        from .. import io as mio

        pattern = f"{self.working_dir}/{self.filename}"
        n_expected = len(glob.glob(pattern))
        seg_off, mol_type, _ = molecule_layout(self.num_mols, self.num_atoms_per_mol)
        # under torch.distributed every rank parses and reduces its own share of the files; the per-frame flux
        # vectors (3 x n_types doubles) are all-gathered in _finish_flux
        files = D.my_files(pattern) if mio.USE_NATIVE_READER else None
        m = q = None
        parts, steps = [], []
        # the charge, ONE more per-atom attribute and the three velocity planes; on the frame stream the fused flux
        # kernel runs on each staging batch while the next one is being parsed (stream.py)
        _, batches = T.attribute_batches(pattern, ("q", "type" if self.mass else "mass"), ("vx", "vy", "vz"),
                                         n_atoms=seg_off[-1], files=files, stream=STREAM, dumps=self.dumps)
        for ts, charge, second, vel in batches:
            if m is None:  # masses and charges of the first frame
                m, q = T.masses(second[0].copy(), self.mass), charge[0].copy()
            parts.append(backend.charge_flux(vel, m, q, seg_off, (mol_type - 1).astype(np.int32), len(self.num_mols),
                                             constants.VELOCITY_CONVERSION[self.units],
                                             constants.CHARGE_CONVERSION[self.units]))
            steps.extend((ts * constants.TIME_CONVERSION[self.units]).tolist())
        flux = np.concatenate(parts, axis=2) if parts else None
        return self._finish_flux(flux, steps, files, n_expected)

    def _finish_flux(self, flux, steps, files, n_expected):
        from .. import dist as D

        if files is not None:
            if flux is None:
                raise ValueError("this rank holds no frame: use at most as many ranks as there are dump files")
            flux = np.moveaxis(D.allgather_var(np.ascontiguousarray(np.moveaxis(flux, 2, 0))), 0, 2)
            steps = list(D.allgather_var(np.asarray(steps, dtype=np.float64)))
        n_frames = 0 if flux is None else flux.shape[2]
        j = np.zeros((3, len(self.num_mols), max(n_expected, n_frames)))
        if flux is not None:
            j[:, :, :n_frames] = flux
        for s in steps:
            self.time.append(s * self.timestep)
        return j

    def correlate_charge_flux(self, flux):
        """tot_flux[i] = sum_j sum_k corr(J[k,i], J[k,j]); last row = sum over i (conductivity.py:197-214)."""
        n_types = len(self.num_mols)
        a = np.stack([flux[k, i] for i in range(n_types) for jj in range(n_types) for k in range(flux.shape[0])])
        b = np.stack([flux[k, jj] for i in range(n_types) for jj in range(n_types) for k in range(flux.shape[0])])
        corr = backend.xcorr(a, b, method=backend.XCORR_FFT).reshape(n_types, n_types * flux.shape[0], -1)
        tot_flux = np.zeros((n_types + 1, flux.shape[2]))
        for i in range(n_types):
            for c in corr[i]:  # same accumulation order as the reference's triple loop
                tot_flux[i, :] += c
                tot_flux[-1, :] += c
        return tot_flux

    def integrate_charge_flux_correlation(self, tot_flux):
        """Running trapezoid integral of every row, first value 0 (conductivity.py:216-232)."""
        delta = self.time[1] - self.time[0]
        return backend.cumtrapz(np.asarray(tot_flux, dtype=np.float64), delta, leading_zero=True)

    def fit_curve(self, tot_flux, integral, tol):
        """Average of each integral over its detected plateau, and the plateau's time range."""
        ave = np.zeros(len(integral))
        time_range = np.zeros(len(integral), dtype=object)
        for i in range(len(integral)):
            lo, hi = self.detect_time_range(tot_flux[i], tol=tol)
            ave[i] = np.average(integral[i][lo:hi])
            time_range[i] = (self.time[lo], self.time[hi])
        return ave, time_range

    def green_kubo(self, ave):
        """sigma = <integral> / (3 kB T V) (conductivity.py:259-274)."""
        return np.array([a / 3 / constants.BOLTZMANN / self.temp / self.volume for a in ave])

    def calc_cond(self, tol=1e-4, plot=False, save=False):
        """
        Whole chain: charge flux, correlation, integral, plateau average, conductivity [S/m] per molecule
        type followed by the total. save writes charge_flux.csv, integral.csv, conductivity.csv; plot
        writes conductivity.png, all into working_dir (conductivity.py:276-397).
        """
        j = self.get_charge_flux()
        tot_flux = self.correlate_charge_flux(j)
        integral = self.integrate_charge_flux_correlation(tot_flux)
        ave, time_range = self.fit_curve(tot_flux, integral, tol)
        cond = self.green_kubo(ave)
        if plot:
            self._plot(tot_flux, integral, time_range)
        if save:
            t = np.array([self.time])
            header = "t," + ",".join(str(i + 1) for i in range(len(tot_flux) - 1)) + ",tot"
            np.savetxt(f"{self.working_dir}/charge_flux.csv", np.append(t, tot_flux, axis=0).T, delimiter=",",
                       header=header, comments="")
            np.savetxt(f"{self.working_dir}/integral.csv", np.append(t, integral, axis=0).T, delimiter=",",
                       header=header, comments="")
            cond = np.asarray([[r[0] for r in time_range], [r[1] for r in time_range], cond])
            np.savetxt(f"{self.working_dir}/conductivity.csv", cond.T, delimiter=",",
                       header="start_t,end_t,cond", comments="")
        return cond

    def _plot(self, tot_flux, integral, time_range):
        import matplotlib

        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt

        from ..utilities.plots import set_axis

        t_ns = np.array(self.time) * 10 ** 9
        cmap = plt.get_cmap("Paired")
        fig, (ax1, ax2) = plt.subplots(1, 2, figsize=(20, 5))
        for i in range(len(tot_flux) - 1):
            ax1.plot(t_ns, tot_flux[i], linewidth=2, color=cmap(i / 10))
            ax2.plot(t_ns, integral[i], linewidth=2, color=cmap(i / 10), label=i + 1)
        ax1.plot(t_ns, tot_flux[-1], linewidth=2, color="black")
        ax2.plot(t_ns, integral[-1], linewidth=2, color="black", label="total")
        ax1.set_ylabel(r"$\mathrm{\langle J(t)\cdot J(0)\rangle}$", fontsize=18)
        ax2.set_ylabel(r"$\mathrm{\int_{0}^{t}\langle J(t')\cdot J(0)\rangle dt'}$", fontsize=18)
        ax2.legend(fontsize=16, loc="center left", bbox_to_anchor=(1, 0.5), frameon=False)
        for ax in (ax1, ax2):
            set_axis(ax, axis="both")
            for edge in time_range[-1]:
                ax.axvline(edge * 10 ** 9, linewidth=2, color="black", linestyle="--")
            ax.set_xscale("log")
            ax.set_xlabel(r"$\mathrm{Time, 10^9 (s)}$", fontsize=18)
        fig.tight_layout(pad=3)
        fig.savefig(f"{self.working_dir}/conductivity.png", bbox_inches="tight", pad_inches=0.1)
        plt.close(fig)

    # ---- Einstein-Helfand / Nernst-Einstein ------------------------------------------------------------------------

    @staticmethod
    def frame_times(steps, time_unit):
        """(order, times [s]) of frames with integer timesteps `steps`: sorted by time; ValueError unless they are equally
        spaced (a lag must be a time)."""
        steps = np.asarray(steps, dtype=np.int64)
        order = np.argsort(steps, kind="stable")
        gaps = np.diff(steps[order])
        if len(gaps) and (gaps[0] <= 0 or np.any(gaps != gaps[0])):
            raise ValueError("the frames are not equally spaced in time (timestep gaps from %d to %d): a lag must be "
                             "a time" % (int(gaps.min()), int(gaps.max())))
        return order, steps[order].astype(np.float64) * time_unit

    def _collective(self):
        """Parses the dumps once per instance: frame times (a separate array: `self.time` belongs to get_charge_flux),
        the collective displacement P [G,3,F] of every molecule type and the per-molecule weighted displacements
        [F,3,M], both on the device."""
        got = getattr(self, "_collective_cache", None)
        if got is not None:
            return got
        import torch

        seg_off, mol_type, _ = molecule_layout(self.num_mols, self.num_atoms_per_mol)
        pattern = f"{self.working_dir}/{self.filename}"

        def missing(lacking, _names):  # the first column the dump lacks; a coordinate only where xu yu zu are not all there
            tail = " (no xu yu zu to use instead)" if lacking[0] in T.WRAPPED else ""
            raise ValueError(f"Missing column '{lacking[0]}' in dump file{tail}.")

        m = q = q_mol = ctx = None
        parts, steps = [], []
        # unsharded: every process reads every file. Whatever the route, each batch is reduced to molecule centres
        # [B,3,M] that stay on the device
        _, batches = T.attribute_batches(pattern, ("q", "type" if self.mass else "mass"), T.UNWRAPPED,
                                         n_atoms=seg_off[-1], stream=STREAM, missing=missing, dumps=self.dumps)
        for ts, charge, second, xyz in batches:
            if m is None:  # masses and charges of the first frame
                m, q = T.masses(second[0].copy(), self.mass), charge[0].copy()
                ctx = backend.default_context()
            out = torch.empty((len(ts), 3, len(seg_off) - 1), dtype=torch.float64,
                              device=torch.device("cuda", ctx.device))
            _, _, seg_q = backend.segment_com(xyz, m, seg_off, atom_q=q, out=out, ctx=ctx)
            if q_mol is None:
                q_mol = seg_q
            parts.append(out)
            steps.extend(ts.tolist())
        if not parts:
            raise ValueError(f"no frames match {pattern}")
        order, times = self.frame_times(steps, constants.TIME_CONVERSION[self.units] * self.timestep)
        com = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
        if np.any(order != np.arange(len(order))):
            com = com.index_select(0, torch.as_tensor(order, device=com.device)).contiguous()
        group_off = np.concatenate(([0], np.cumsum(self.num_mols))).astype(np.int64)
        F, _, M = com.shape
        P = torch.empty((len(self.num_mols), 3, F), dtype=torch.float64, device=com.device)
        weighted = torch.empty((F, 3, M), dtype=torch.float64, device=com.device)
        backend.collective_displacement(com, np.asarray(q_mol) * constants.CHARGE_CONVERSION[self.units], group_off,
                                        scale=constants.DISTANCE_CONVERSION[self.units], out=P, weighted=weighted)
        self._collective_cache = {"times": times, "P": P, "weighted": weighted, "group_off": group_off}
        return self._collective_cache

    @staticmethod
    def fit_window(lag_times, initial_time=None, final_time=None):
        """(first, last) lag index of the fit, both included: the lags with initial_time <= t <= final_time [s]; a
        missing end defaults to 20 % (rounded up) / 80 % (rounded down) of max_lag = len(lag_times) - 1."""
        lag_times = np.asarray(lag_times, dtype=np.float64)
        max_lag = len(lag_times) - 1
        lo = -(-max_lag // 5) if initial_time is None else int(np.searchsorted(lag_times, initial_time, side="left"))
        hi = (4 * max_lag) // 5 if final_time is None else int(np.searchsorted(lag_times, final_time, side="right")) - 1
        if hi - lo < 1:
            raise ValueError("the fit window [%r, %r] holds fewer than two of the %d lags" % (initial_time, final_time,
                                                                                          max_lag + 1))
        return lo, hi

    @staticmethod
    def fit_weights(t):
        """w with slope = w @ y: the ordinary least-squares line with intercept through (t, y)."""
        t = np.asarray(t, dtype=np.float64)
        c = t - t.mean()
        return c / np.sum(c * c)

    def helfand(self, slope):
        """sigma = slope / (6 kB T V)."""
        return np.asarray(slope) / 6 / constants.BOLTZMANN / self.temp / self.volume

    def _lag_range(self, n_frames, max_lag):
        max_lag = (n_frames - 1) // 2 if max_lag is None else int(max_lag)
        if not 1 <= max_lag <= n_frames - 1:
            raise ValueError("max_lag must be in [1, n_frames - 1 = %d]" % (n_frames - 1))
        return max_lag

    def _finish_helfand(self, name, t, cols, lo, hi, cond, save, plot):
        """The table `t, 1, ..., tot` of a method and what save / plot write for it."""
        n_types = len(self.num_mols)
        table = pd.DataFrame(dict([("t", t)] + [(str(i + 1), cols[i]) for i in range(n_types)] + [("tot", cols[-1])]))
        if save:
            header = "t," + ",".join(str(i + 1) for i in range(n_types)) + ",tot"
            np.savetxt(f"{self.working_dir}/{name}_msd.csv", table.to_numpy(), delimiter=",", header=header, comments="")
            rows = np.asarray([[t[lo]] * len(cond), [t[hi]] * len(cond), cond])
            np.savetxt(f"{self.working_dir}/{name}_conductivity.csv", rows.T, delimiter=",",
                       header="start_t,end_t,cond", comments="")
        if plot:
            self._plot_helfand(name, t, cols, (t[lo], t[hi]))
        return table

    def einstein(self, max_lag=None, initial_time=None, final_time=None, save=False, plot=False):
        """
        Einstein-Helfand conductivity [S/m] per molecule type followed by the total: sigma_ab = slope of
        <dP_a(t) . dP_b(t)> / (6 kB T V), P_a the charge-weighted collective displacement of type a; element i is
        sum_b sigma_ib (the convention of calc_cond). Lags 0 .. max_lag frames (default (F - 1) // 2); the line is fitted
        over [initial_time, final_time] seconds (default: lags from 20 % to 80 % of max_lag). Keeps `self.onsager`
        (sigma_ab) and `self.einstein_msd` (t, one column per type: the row sum, tot). save writes einstein_msd.csv and
        einstein_conductivity.csv, plot writes einstein.png, into working_dir.
        """
        col = self._collective()
        times = col["times"]
        max_lag = self._lag_range(len(times), max_lag)
        out = backend.cross_msd(col["P"], max_lag)
        t = times[: max_lag + 1] - times[0]
        lo, hi = self.fit_window(t, initial_time, final_time)
        w = self.fit_weights(t[lo:hi + 1])
        self.onsager = self.helfand(np.tensordot(w, out[lo:hi + 1], axes=(0, 0)))
        cond = np.append(self.onsager.sum(axis=1), self.onsager.sum())
        cols = [out[:, a, :].sum(axis=1) for a in range(out.shape[1])] + [out.sum(axis=(1, 2))]
        self.einstein_msd = self._finish_helfand("einstein", t, cols, lo, hi, cond, save, plot)
        self._einstein_cond = cond
        return cond

    def nernst(self, max_lag=None, initial_time=None, final_time=None, save=False, plot=False):
        """
        Nernst-Einstein conductivity [S/m] per molecule type followed by the total: the self part of `einstein`,
        S_a(t) = sum over the molecules e of type a of c_e^2 <|dr_e(t)|^2>, same lags, fit and factor. Keeps
        `self.nernst_msd`; save writes nernst_msd.csv and nernst_conductivity.csv, plot writes nernst.png.
        """
        col = self._collective()
        times = col["times"]
        max_lag = self._lag_range(len(times), max_lag)
        msd = backend.lag_msd(col["weighted"], max_lag, col["group_off"], scale=1.0)
        size = np.diff(col["group_off"]).astype(np.float64)
        self_part = np.where(size > 0, msd[:, :, 3] * size, 0.0)  # [lag, type]: mean over molecules -> sum
        t = times[: max_lag + 1] - times[0]
        lo, hi = self.fit_window(t, initial_time, final_time)
        w = self.fit_weights(t[lo:hi + 1])
        sigma = self.helfand(w @ self_part[lo:hi + 1])
        cond = np.append(sigma, sigma.sum())
        cols = [self_part[:, a] for a in range(self_part.shape[1])] + [self_part.sum(axis=1)]
        self.nernst_msd = self._finish_helfand("nernst", t, cols, lo, hi, cond, save, plot)
        self._nernst_cond = cond
        return cond

    def ionicity(self):
        """sigma_Einstein / sigma_Nernst-Einstein of the whole system; computes whichever is missing with its defaults."""
        if getattr(self, "_einstein_cond", None) is None:
            self.einstein()
        if getattr(self, "_nernst_cond", None) is None:
            self.nernst()
        return self._einstein_cond[-1] / self._nernst_cond[-1]

    def _plot_helfand(self, name, t, cols, window):
        import matplotlib

        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt

        from ..utilities.plots import set_axis

        t_ns = np.asarray(t) * 10 ** 9
        cmap = plt.get_cmap("Paired")
        fig, ax = plt.subplots(1, 1, figsize=(10, 5))
        for i in range(len(cols) - 1):
            ax.plot(t_ns, cols[i], linewidth=2, color=cmap(i / 10), label=i + 1)
        ax.plot(t_ns, cols[-1], linewidth=2, color="black", label="total")
        for edge in window:
            ax.axvline(edge * 10 ** 9, linewidth=2, color="black", linestyle="--")
        set_axis(ax, axis="both")
        ax.set_xlabel(r"$\mathrm{Time, 10^9 (s)}$", fontsize=18)
        ax.set_ylabel(r"$\mathrm{\langle \Delta P(t)\cdot \Delta P(t)\rangle, C^2 m^2}$", fontsize=18)
        ax.legend(fontsize=16, loc="center left", bbox_to_anchor=(1, 0.5), frameon=False)
        fig.tight_layout(pad=3)
        fig.savefig(f"{self.working_dir}/{name}.png", bbox_inches="tight", pad_inches=0.1)
        plt.close(fig)
