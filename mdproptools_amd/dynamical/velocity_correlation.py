"""
Velocity autocorrelation function (VACF), vibrational density of states (VDOS) and the Green-Kubo self-diffusion
coefficient from the velocities of a LAMMPS trajectory,

    vacf(k) = < v_e(t) . v_e(t + k) >   over the entities e of a group and the time origins t,
    vdos(f) ~ the Fourier transform of the (windowed) vacf,        D = (1/3) * integral of vacf dt.

The reference has no such module; the constructor follows `Diffusion` and `Conductivity` for `timestep`, `units` and
`mass`, the tables and plots follow `Reorientation`.

What runs where
  GPU (libmdhip.so): `vel_type="com"` reduces every batch of frames to molecular centre-of-mass velocities
      (`mdhip_segment_com`, which is linear); the velocities [F,3,E] stay on the device; `mdhip_velocity_spectrum`
      gives the lag sums and the power spectrum of every group — atom types (interleaved inside molecules) or molecule
      types — in one pass over them; the running integral of the diffusion coefficient is `mdhip_cumtrapz`.
  Host: parsing (common/trajectory.py: the frames are never all resident), the order and spacing of the frames, the
      normalisations, the lag window and its short transform (one series of at most 2 max_lag + 2 points per group), the
      CSV / PNG files.

The class is single process: every process that constructs one reads every file. Sharding over `torch.distributed` is
out of scope here.
"""

import glob
import os

import numpy as np
import pandas as pd

from .. import backend
from ..common import constants
from ..common import trajectory as T
from ..common.com_mols import molecule_layout
from ..dist import is_writer

# True: the dumps are parsed into page-locked staging batches and each is moved (or reduced) to the GPU while the next
# one is being parsed (mdproptools_amd/stream.py). False: every frame is parsed first.
STREAM = True
BATCH_BYTES = None  # bytes of velocities per streamed batch (None: the stream's own default)

MAX_GROUPS = backend.VELOCITY_MAX_GROUPS
THZ = 1e12
LIGHT_SPEED_CM = 2.99792458e10  # cm / s: wavenumber = frequency / c


class VelocityCorrelation:
    def __init__(self, filename, vel_type="allatom", num_mols=None, num_atoms_per_mol=None, mass=None, timestep=1,
                 units="real", weighting=None, working_dir=None):
        """
        filename: dump file or '*' pattern (relative to working_dir unless absolute) with the columns id, type, vx, vy,
        vz (and mass, when masses are needed and `mass` is None). vel_type "allatom": one group per atom type of the
        dump's `type` column (at most 16); "com": centre-of-mass velocities of the molecules given by num_mols /
        num_atoms_per_mol (molecules per type and atoms per molecule in id order), one group per molecule type.
        mass: per-atom-type masses, or None to read the dump's mass column; timestep in the time unit of `units` (LAMMPS
        unit style). weighting None: plain velocities; "mass": the series are sqrt(m) * v, so that the spectrum is the
        mass-weighted one (the results then carry the mass unit of `units` as a factor). working_dir: where the dumps
        are and the CSV files go (default: the current directory; `self.save_mode = False` writes none).
        `self.normalize = False` keeps the VDOS columns unnormalised. The dumps are read on first use. Single process.
        """
        if units not in constants.SUPPORTED_UNITS:
            raise KeyError("Unit type not supported. Supported units are: " + str(constants.SUPPORTED_UNITS))
        if vel_type not in ("allatom", "com"):
            raise ValueError("vel_type must be 'allatom' or 'com'.")
        if weighting not in (None, "mass"):
            raise ValueError("weighting must be None or 'mass'.")
        if vel_type == "com":
            if num_mols is None or num_atoms_per_mol is None or len(num_mols) != len(num_atoms_per_mol) or not len(num_mols):
                raise ValueError("vel_type 'com' needs num_mols and num_atoms_per_mol, one entry per molecule type")
            if len(num_mols) > MAX_GROUPS:
                raise ValueError("at most %d molecule types (%d given)" % (MAX_GROUPS, len(num_mols)))
        self.filename = filename
        self.vel_type = vel_type
        self.num_mols = num_mols
        self.num_atoms_per_mol = num_atoms_per_mol
        self.mass = mass
        self.timestep = timestep
        self.units = units
        self.weighting = weighting
        self.working_dir = working_dir or os.getcwd()
        self.save_mode = True
        self.normalize = True
        self.vacf_df = None
        self.vdos_df = None
        self.gk_df = None
        self.diff_df = None
        self._traj = None
        self._sums = None  # (max_lag, sums [max_lag+1,G,4]) of the last call

    # ---- the velocities -----------------------------------------------------------------------------------------------

    @staticmethod
    def group_table(types):
        """(labels, ent_group int32 [E], counts) of per-entity type numbers: one group per distinct type, ascending."""
        types = np.asarray(types)
        labels, index = np.unique(types.astype(np.int64), return_inverse=True)
        if len(labels) > MAX_GROUPS:
            raise ValueError("at most %d groups per instance (the dump has %d types)" % (MAX_GROUPS, len(labels)))
        return [int(t) for t in labels], index.astype(np.int32), np.bincount(index, minlength=len(labels)).astype(np.int64)

    def _load(self):
        """(v [F,3,E] float64 CUDA tensor, frames in time order; times [F] in s; labels; ent_group int32 [E]; counts [G];
        coef [E] or None): read once per instance."""
        if self._traj is not None:
            return self._traj
        import torch

        from .conductivity import Conductivity

        com = self.vel_type == "com"
        need_mass = com or self.weighting == "mass"
        seg = molecule_layout(self.num_mols, self.num_atoms_per_mol) if com else None
        pattern = self.filename if os.path.isabs(self.filename) else f"{self.working_dir}/{self.filename}"

        def missing(lacking, _names):
            raise ValueError(f"Missing column '{lacking[0]}' in dump file.")

        # id, ONE more per-atom attribute, the three velocity planes — except where the atoms' types AND the dump's masses
        # are needed: type and mass then (the frames come ordered by id either way)
        type_first = not com and need_mass and not self.mass
        leading = ("type", "mass") if type_first else ("id", ("type" if self.mass else "mass") if com else "type")
        streamed, batches = T.attribute_batches(pattern, leading, ("vx", "vy", "vz"), n_atoms=seg[0][-1] if com else None,
                                                stream=STREAM, batch_bytes=BATCH_BYTES, missing=missing)
        types0 = second0 = atom_mass = seg_mass = ctx = dev = v = None
        steps = []
        for ts, first, second, vel in batches:
            types = first if type_first else second  # (allatom; 'com' groups by the layout)
            if second0 is None:  # (the context only once there is a frame: a dump that lacks a column is refused before)
                ctx = backend.default_context()
                dev = torch.device("cuda", ctx.device)
                types0, second0 = types[0].copy(), second[0].copy()
                atom_mass = np.asarray(T.masses(second0, self.mass), dtype=np.float64) if need_mass else None
                # ONE tensor for the whole trajectory, sized by the files (one frame each, as a rule) and doubled when a
                # file holds more: the batches are written where they stay, no second copy to join them
                n_ent = len(seg[0]) - 1 if com else vel.shape[2]
                v = torch.empty((max(len(glob.glob(pattern)), len(ts)), 3, n_ent), dtype=torch.float64, device=dev)
            if not com and not (types == types0).all():
                raise ValueError("atom types change between frames")
            if need_mass and not (second == second0).all() and not (T.masses(second, self.mass) == atom_mass).all():
                raise ValueError("atom masses change between frames")
            n = len(steps)
            if n + len(ts) > v.shape[0]:
                grown = torch.empty((max(2 * v.shape[0], n + len(ts)),) + tuple(v.shape[1:]), dtype=torch.float64, device=dev)
                grown[:n].copy_(v[:n])
                v = grown
            out = v[n:n + len(ts)]
            if com:
                _, seg_mass, _ = backend.segment_com(vel, atom_mass, seg[0], out=out, ctx=ctx)
            else:
                out.copy_(torch.from_numpy(np.ascontiguousarray(vel)))  # (a staging batch is reused: what is kept is a copy)
            steps.extend(np.asarray(ts).tolist())
        if not steps:
            raise ValueError("need at least one array to stack")  # (no frame at all: numpy's words for it, as Diffusion)
        order, times = Conductivity.frame_times(steps, self.timestep * constants.TIME_CONVERSION[self.units])
        v = v[:len(steps)]
        if not np.array_equal(order, np.arange(len(order))):  # (files out of time order: the one case with a second copy)
            v = v[torch.as_tensor(order, device=dev)].contiguous()
        if com:
            labels, ent_group, counts = self.group_table(seg[1])
            ent_mass = np.asarray(seg_mass, dtype=np.float64)
        else:
            labels, ent_group, counts = self.group_table(types0)
            ent_mass = atom_mass
        coef = np.sqrt(ent_mass) if self.weighting == "mass" else None
        self._traj = (v, times, labels, ent_group, counts, coef)
        return self._traj

    def _lag_sums(self, max_lag):
        """(max_lag, sums [max_lag+1,G,4]) from the library, kept for the methods that follow."""
        v, times, _, ent_group, _, coef = self._load()
        F = len(times)
        max_lag = (F - 1) // 2 if max_lag is None else int(max_lag)
        if not 0 <= max_lag <= F - 1:
            raise ValueError("max_lag must be in [0, %d] (the trajectory has %d frames)" % (F - 1, F))
        if self._sums is None or self._sums[0] != max_lag:
            sums, _, _ = backend.velocity_spectrum(v, ent_group, max_lag, coef=coef)
            self._sums = (max_lag, np.asarray(sums))
        return self._sums

    def _conversion(self):
        return constants.VELOCITY_CONVERSION[self.units] ** 2

    # ---- VACF ---------------------------------------------------------------------------------------------------------

    def calc_vacf(self, max_lag=None, plot=False):
        """The VACF of every group at the lags 0 .. max_lag frames (default (F - 1) // 2): a DataFrame `Time (s)` and, per
        group label i, `vacf_x{i}`, `vacf_y{i}`, `vacf_z{i}`, `vacf{i}` = the lag sums / ((F - k) * N_i) in m^2/s^2 (the
        last one the sum over the axes: <v(0) . v(t)>) and `cvv{i}` = vacf{i}(t) / vacf{i}(0). Kept in `self.vacf_df`
        and, with save_mode, written to vacf.csv (plot: vacf.png) in working_dir."""
        _, times, labels, _, counts, _ = self._load()
        max_lag, sums = self._lag_sums(max_lag)
        cols = {"Time (s)": times[: max_lag + 1] - times[0]}
        origins = (len(times) - np.arange(max_lag + 1)).astype(np.float64)
        conv = self._conversion()
        for g, lab in enumerate(labels):
            w = origins * float(counts[g])
            with np.errstate(invalid="ignore", divide="ignore"):
                for a, name in enumerate(("vacf_x", "vacf_y", "vacf_z", "vacf")):
                    cols["%s%d" % (name, lab)] = sums[:, g, a] / w * conv
                cols["cvv%d" % lab] = cols["vacf%d" % lab] / cols["vacf%d" % lab][0]
        self.vacf_df = pd.DataFrame(cols)
        if self.save_mode and is_writer():
            self.vacf_df.to_csv(self.working_dir + "/vacf.csv")
        if plot and is_writer():
            self._plot(self.vacf_df, "Time (s)", "cvv", r"$\mathrm{Time, s}$", r"$\mathrm{C_{vv}(t)}$", "vacf.png")
        return self.vacf_df

    # ---- VDOS ---------------------------------------------------------------------------------------------------------

    def calc_vdos(self, max_lag=None, window="hann", n_freq=None, plot=False):
        """The vibrational density of states of every group: a DataFrame `Frequency (THz)`, `Wavenumber (cm^-1)` and
        `vdos{i}` per group label.
        window "hann" or "none": the lag-window estimate dt * (c(0) + 2 sum_{k=1..M} c(k) cos(2 pi j k / n_freq)),
        c(k) = w(k) * vacf{i}(k), w(k) = 0.5 (1 + cos(pi k / M)) or 1, M = max_lag (default (F - 1) // 2), at the
        frequencies j / (n_freq dt), j = 0 .. n_freq / 2; n_freq a power of two >= 2 M + 2 (default: the smallest).
        window None: the raw periodogram dt * power_total / (F * N_i) * conversion at j / (L dt), L the library's padded
        length (max_lag and n_freq are not used).
        Every column is normalised to unit area by the trapezoid rule over the frequency axis (in Hz) unless
        `self.normalize` is False. Kept in `self.vdos_df`; with save_mode written to vdos.csv (plot: vdos.png)."""
        if window not in ("hann", "none", None):
            raise ValueError("window must be 'hann', 'none' or None")
        v, times, labels, ent_group, counts, coef = self._load()
        F = len(times)
        if F < 2:
            raise ValueError("a spectrum needs at least two frames")
        dt = float(times[1] - times[0])
        conv = self._conversion()
        spectra = {}
        if window is None:
            _, power, _ = backend.velocity_spectrum(v, ent_group, 0, coef=coef, want_power=True)
            power = np.asarray(power)
            L = 2 * (power.shape[2] - 1)
            freq = np.arange(L // 2 + 1) / (L * dt)
            for g, lab in enumerate(labels):
                with np.errstate(invalid="ignore", divide="ignore"):
                    spectra[lab] = dt * power[g, 3] / (F * float(counts[g])) * conv
        else:
            max_lag, sums = self._lag_sums(max_lag)
            M = max_lag
            smallest = 4
            while smallest < 2 * M + 2:
                smallest *= 2
            n_freq = smallest if n_freq is None else int(n_freq)
            if n_freq < 2 * M + 2 or n_freq & (n_freq - 1):
                raise ValueError("n_freq must be a power of two >= 2 * max_lag + 2 = %d" % (2 * M + 2))
            k = np.arange(M + 1)
            w = 0.5 * (1.0 + np.cos(np.pi * k / M)) if window == "hann" and M > 0 else np.ones(M + 1)
            origins = (F - k).astype(np.float64)
            freq = np.arange(n_freq // 2 + 1) / (n_freq * dt)
            for g, lab in enumerate(labels):
                with np.errstate(invalid="ignore", divide="ignore"):
                    c = w * (sums[:, g, 3] / (origins * float(counts[g])) * conv)
                even = np.zeros(n_freq)  # the even extension c(-k) = c(k): its transform is the cosine sum, real
                even[: M + 1] = c
                even[n_freq - M:] = c[1:][::-1]
                spectra[lab] = dt * np.fft.rfft(even).real
        cols = {"Frequency (THz)": freq / THZ, "Wavenumber (cm^-1)": freq / LIGHT_SPEED_CM}
        for lab in labels:
            s = spectra[lab]
            if self.normalize:
                area = float(np.sum(0.5 * (s[1:] + s[:-1]) * np.diff(freq)))
                with np.errstate(invalid="ignore", divide="ignore"):
                    s = s / area
            cols["vdos%d" % lab] = s
        self.vdos_df = pd.DataFrame(cols)
        if self.save_mode and is_writer():
            self.vdos_df.to_csv(self.working_dir + "/vdos.csv")
        if plot and is_writer():
            self._plot(self.vdos_df, "Frequency (THz)", "vdos", r"$\mathrm{Frequency, THz}$", r"$\mathrm{VDOS}$", "vdos.png")
        return self.vdos_df

    # ---- Green-Kubo diffusion -------------------------------------------------------------------------------------------

    def calc_diffusion(self, t_cut=None):
        """The Green-Kubo self-diffusion coefficient of every group: one row per group, `D (m^2/s)` = (1/3) times the
        trapezoid integral of vacf{i} from 0 to t_cut (s; default: the last lag of the VACF table, which is computed with
        its defaults when there is none yet; a given t_cut is rounded down to a lag). The running integral (1/3 included)
        is kept in `self.gk_df`, the rows in `self.diff_df`; with save_mode written to diffusion_gk.csv."""
        if self.weighting == "mass":
            raise ValueError("the integral of the mass-weighted VACF is not a diffusion coefficient: use weighting=None")
        if self.vacf_df is None:
            self.calc_vacf()
        _, _, labels, _, counts, _ = self._load()
        t = self.vacf_df["Time (s)"].to_numpy(dtype=np.float64)
        n = len(t)
        names = ["vacf%d" % lab for lab in labels]
        Y = np.ascontiguousarray(self.vacf_df[names].to_numpy(dtype=np.float64).T)
        dx = float(t[1] - t[0]) if n > 1 else 1.0
        running = np.asarray(backend.cumtrapz(Y, dx, leading_zero=True)).reshape(len(names), n) / 3.0 if n > 1 else \
            np.zeros((len(names), n))
        i_cut = n - 1 if t_cut is None else int(np.clip(np.searchsorted(t, float(t_cut), side="right") - 1, 0, n - 1))
        self.gk_df = pd.DataFrame(dict({"Time (s)": t}, **{"D%d" % lab: running[g] for g, lab in enumerate(labels)}))
        self.diff_df = pd.DataFrame({"group": labels, "N": [int(c) for c in counts], "t_cut (s)": float(t[i_cut]),
                                     "D (m^2/s)": [float(running[g, i_cut]) for g in range(len(labels))]})
        if self.save_mode and is_writer():
            self.diff_df.to_csv(self.working_dir + "/diffusion_gk.csv")
        return self.diff_df

    # ---- plots ----------------------------------------------------------------------------------------------------------

    def _plot(self, df, x_name, prefix, x_label, y_label, file_name):
        import matplotlib

        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt

        from ..utilities.plots import set_axis

        x = df[x_name].to_numpy()
        cmap = plt.get_cmap("Paired")
        fig, ax = plt.subplots(1, 1, figsize=(10, 5))
        labels = self._load()[2]
        for i, lab in enumerate(labels):
            ax.plot(x, df["%s%d" % (prefix, lab)], linewidth=2, color=cmap((i % 12) / 12), label=str(lab))
        ax.axhline(0.0, linewidth=1, color="black", linestyle="--")
        set_axis(ax, axis="both")
        ax.set_xlabel(x_label, fontsize=18)
        ax.set_ylabel(y_label, fontsize=18)
        ax.legend(fontsize=16, loc="center left", bbox_to_anchor=(1, 0.5), frameon=False)
        fig.tight_layout(pad=3)
        fig.savefig(f"{self.working_dir}/{file_name}", bbox_inches="tight", pad_inches=0.1)
        plt.close(fig)
