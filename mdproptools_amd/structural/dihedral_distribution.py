"""
Dihedral (torsion) angles inside molecules from LAMMPS dumps: their distributions and conformer populations — the
cis / trans populations of TFSI (C-S-N-S), the gauche / trans statistics of the O-C-C-O and C-O-C-C torsions of glymes,
carbonates and PEO — and the torsional autocorrelation function, which tells how fast the conformers interconvert. The
reference has no such module; include/mdhip.h (mdhip_dihedral_angles) holds the specification and
tests/dihedral_ref.py restates it in numpy. Arguments follow `Reorientation` and `calc_angular_distribution`.

What runs where
  GPU (libmdhip.so, csrc/dihedrals.hip): per frame, molecule and quadruple the torsion as (cos phi, sin phi), its bin
      and exact integer histograms per entry, or the series U [S,3,F] = (cos phi, sin phi, 0), which stay on the device;
      `mdhip_orient_corr` then sums u(t) . u(t+k) = cos(phi(t+k) - phi(t)) over molecules and origins at every lag.
  Host: parsing (common/trajectory.py: the frames are never all resident), the molecule layout, the cosine table of
      the bin edges, adding the batches' integer histograms, normalisation, populations and the CSV files.

The angle follows the IUPAC convention: cis = 0, trans = +-180, the sign by the right-hand rule about j -> k. Bins
cover [-180, 180) in steps of bin_size and mirror each other about 0: the positive half is left-closed, the negative
half right-closed (an angle of exactly -60 counts in (-61, -60] at bin_size = 1), exactly 0 and exactly 180 count on the
positive side. With wrapped coordinates every bond difference i-j, j-k, k-l is wrapped once on its own, which is right
whenever consecutive named atoms lie within half a box edge of each other, as bonded atoms do.
"""

import os

import numpy as np
import pandas as pd

from .. import backend
from ..common import mol_series
from ..common.tables import density
from ..common.trajectory import refuse_triclinic
from ..dist import is_writer

# True: the dumps are parsed into page-locked staging batches and each is reduced on the GPU while the next one is
# being parsed (mdproptools_amd/stream.py). False: every frame is parsed first and reduced in one call.
STREAM = True
BATCH_BYTES = None  # bytes of coordinates per streamed batch (None: the stream's own default)

MAX_DIHEDRALS = backend.DIHEDRAL_MAX_ROWS
MIN_BIN_SIZE = 360.0 / backend.DIHEDRAL_MAX_BINS
DEFAULT_STATES = {"g-": (-120, 0), "g+": (0, 120), "t": (120, -120)}


def _checked(dihedrals, atoms_per_mol):
    """[(mol_type, [(i, j, k, l), ...] 1-based, label)] of the entries, or a ValueError that names the bad one."""
    dihedrals = list(dihedrals)
    if not dihedrals:
        raise ValueError("dihedrals must name at least one (mol_type, i, j, k, l) or (mol_type, [(i, j, k, l), ...])")
    if len(dihedrals) > MAX_DIHEDRALS:
        raise ValueError("at most %d dihedrals per call (%d given)" % (MAX_DIHEDRALS, len(dihedrals)))
    out = []
    for d in dihedrals:
        d = tuple(d)
        label = None
        if len(d) == 5:
            quads = [d[1:]]
        elif len(d) in (2, 3) and not isinstance(d[1], (str, bytes)) and np.ndim(d[1]) == 2:
            quads = [tuple(q) for q in d[1]]
            if len(d) == 3:
                if not isinstance(d[2], str) or not d[2]:
                    raise ValueError("dihedral %r: the label must be a non-empty string" % (d,))
                label = d[2]
        else:
            raise ValueError("a dihedral is (mol_type, i, j, k, l), (mol_type, [(i, j, k, l), ...]) or "
                             "(mol_type, [(i, j, k, l), ...], label): %r" % (d,))
        mol_type = int(d[0])
        if not 1 <= mol_type <= len(atoms_per_mol):
            raise ValueError("dihedral %r: mol_type must be in [1, %d]" % (d, len(atoms_per_mol)))
        n = atoms_per_mol[mol_type - 1]
        if not quads:
            raise ValueError("dihedral %r: no quadruple" % (d,))
        checked = []
        for q in quads:
            if len(q) != 4:
                raise ValueError("dihedral %r: a quadruple is four atoms (i, j, k, l)" % (d,))
            q = tuple(int(v) for v in q)
            if not all(1 <= v <= n for v in q):
                raise ValueError("dihedral %r: the atoms must be in [1, %d], the atoms of a molecule of type %d"
                                 % (d, n, mol_type))
            if len(set(q)) != 4:
                raise ValueError("dihedral %r: an atom is named twice" % (d,))
            checked.append(q)
        if label is None:
            label = "%d:%d-%d-%d-%d" % ((mol_type,) + checked[0]) + ("+%d" % (len(checked) - 1) if len(checked) > 1 else "")
        if any(label == other[2] for other in out):
            raise ValueError("dihedral %r: the label %r is taken; give the entry a label of its own" % (d, label))
        out.append((mol_type, checked, label))
    return out


def _jobs(entries, num_mols, num_atoms_per_mol):
    """(job_atom0, job_mols, job_len, quads [J,4] 0-based, job_row) of the entries: one job per quadruple over all
    molecules of its type, the jobs of an entry in a row and adding to the entry's histogram row."""
    rows = [e for e, (_, quads, _) in enumerate(entries) for _ in quads]
    quads = [[v - 1 for v in q] for _, qs, _ in entries for q in qs]
    return mol_series.type_jobs([entries[e][0] - 1 for e in rows], num_mols, num_atoms_per_mol) + (
        np.asarray(quads, dtype=np.int32), np.asarray(rows, dtype=np.int32))


def _n_bins(bin_size):
    bin_size = float(bin_size)
    half = 180.0 / bin_size if bin_size > 0 else 0.0
    if not (bin_size >= MIN_BIN_SIZE and half >= 1 and abs(half - round(half)) <= 1e-9 * half):
        raise ValueError("bin_size must divide 180 degrees into a whole number of bins and be at least %g (%r given)"
                         % (MIN_BIN_SIZE, bin_size))
    return 2 * int(round(half))


def _state_bins(states, n_bins):
    """name -> (first bin, bin behind the last one, wraps) of the windows (lo, hi) in degrees."""
    D = 360.0 / n_bins
    out = {}
    for name, window in states.items():
        try:
            lo, hi = (float(v) for v in window)
        except (TypeError, ValueError):
            raise ValueError("state %r must be (lo, hi) in degrees" % (name,)) from None
        b = [(v + 180.0) / D for v in (lo, hi)]
        if not all(-180.0 <= v <= 180.0 for v in (lo, hi)) or any(abs(v - round(v)) > 1e-9 * n_bins for v in b) or lo == hi:
            raise ValueError("state %r: lo and hi must be different multiples of bin_size within [-180, 180] (%r given)"
                             % (name, tuple(window)))
        out[str(name)] = (int(round(b[0])), int(round(b[1])), lo > hi)
    if not out:
        raise ValueError("states must name at least one window")
    return out


def _prepare(dihedrals, filename, num_mols, num_atoms_per_mol, coords):
    if coords not in ("wrapped", "unwrapped"):
        raise ValueError('coords must be "wrapped" or "unwrapped"')
    num_mols, per = mol_series.layout(num_mols, num_atoms_per_mol)
    entries = _checked(dihedrals, per)
    return entries, num_mols, per


def calc_dihedral_distribution(dihedrals, filename, num_mols, num_atoms_per_mol, bin_size=1.0, states=None,
                               coords="wrapped", save_mode=True, working_dir=None):
    """
    Distributions of the dihedral angles `dihedrals` over the frames of `filename` (dump file or '*' pattern).
    dihedrals: a list of at most 16 entries (mol_type, i, j, k, l), (mol_type, [(i, j, k, l), ...]) or
    (mol_type, [(i, j, k, l), ...], "label") — mol_type the 1-based index into num_mols, the atoms 1-based inside the
    molecule; the quadruples of one entry are pooled into one distribution (the five O-C-C-O torsions of a tetraglyme).
    The default label is `type:i-j-k-l`, `type:i-j-k-l+N` with N further quadruples.
    num_mols / num_atoms_per_mol: molecules per type and atoms per molecule in id order. bin_size: degrees; it must
    divide 180 into a whole number of bins and be at least 0.25. states: name -> (lo, hi) in degrees, multiples of
    bin_size, lo > hi wrapping through +-180 (default: g- (-120, 0), g+ (0, 120), t (120, -120)). coords="wrapped" reads
    `x y z` and the box, coords="unwrapped" `xu yu zu` (or x y z ix iy iz). Triclinic boxes are not supported.

    Returns (dist_df, pop_df):
      dist_df: `phi (deg)` (bin centres from -180 + bin_size / 2) and per entry `p_<label>` = counts / (total * bin_size)
        (integrates to 1 over degrees; NaN for an entry without counts);
      pop_df: one row per entry: `dihedral` (the label), one column per state (the share of the counts in its whole
        bins, a ratio of integer sums), `n` (the counted angles) and `n_degenerate` (quadruples with three collinear
        atoms, which have no angle).
    With save_mode they are written to dihedral_distribution.csv and dihedral_populations.csv in working_dir (default:
    the current directory).
    """
    entries, num_mols, per = _prepare(dihedrals, filename, num_mols, num_atoms_per_mol, coords)
    n_bins = _n_bins(bin_size)
    D = 360.0 / n_bins
    windows = _state_bins(DEFAULT_STATES if states is None else states, n_bins)
    refuse_triclinic(filename)
    a0, mols, length, quads, rows = _jobs(entries, num_mols, per)
    E = len(entries)
    hist = np.zeros((E, n_bins), dtype=np.uint64)

    def compute(xyz, box, _out, _ctx, _ids):
        h, _, deg = backend.dihedral_angles(xyz, box, a0, mols, length, quads, job_row=rows, n_bins=n_bins)
        np.add(hist, h, out=hist)
        return deg

    degenerate = mol_series.load_series(filename, coords, int(np.dot(num_mols, per)), compute, mols, rows, E,
                                        stream=STREAM, batch_bytes=BATCH_BYTES)[3]

    dist = {"phi (deg)": -180.0 + D / 2 + D * np.arange(n_bins)}
    pops = []
    for e, (_, _, label) in enumerate(entries):
        cnt = hist[e].astype(np.int64)
        total = int(cnt.sum())
        dist["p_" + label] = density(cnt, D)
        row = {"dihedral": label}
        for name, (b0, b1, wraps) in windows.items():
            inside = int(cnt[b0:].sum() + cnt[:b1].sum()) if wraps else int(cnt[b0:b1].sum())
            row[name] = inside / total if total else np.nan
        row["n"], row["n_degenerate"] = total, int(degenerate[e])
        pops.append(row)
    dist_df, pop_df = pd.DataFrame(dist), pd.DataFrame(pops, columns=["dihedral"] + list(windows) + ["n", "n_degenerate"])
    if save_mode and is_writer():
        where = working_dir or os.getcwd()
        dist_df.to_csv(where + "/dihedral_distribution.csv")
        pop_df.to_csv(where + "/dihedral_populations.csv")
    return dist_df, pop_df


def _refuse_degenerate(entries, degenerate):
    """A torsion that does not exist has no correlation function."""
    mol_series.refuse_degenerate([e[2] for e in entries], degenerate, "degenerate dihedrals",
                                 "Three of the four atoms are collinear or coincide there")


def _load_series(entries, filename, num_mols, per, dt, coords):
    """(U [S,3,F] float64 CUDA tensor = (cos phi, sin phi, 0), frames in time order; times [F] in ps; group_off [E+1];
    degenerate uint64 [E])."""
    a0, mols, length, quads, rows = _jobs(entries, num_mols, per)

    def compute(xyz, box, out, ctx, _ids):
        return backend.dihedral_angles(xyz, box, a0, mols, length, quads, out=out, ctx=ctx)[2]

    return mol_series.load_series(filename, coords, int(np.dot(num_mols, per)), compute, mols, rows, len(entries),
                                  dt * 10 ** -3, stream=STREAM, batch_bytes=BATCH_BYTES)  # dt in fs, as Reorientation


def calc_dihedral_correlation(dihedrals, filename, num_mols, num_atoms_per_mol, dt=1, max_lag=None, coords="wrapped",
                              save_mode=True, working_dir=None):
    """
    The torsional autocorrelation functions of `dihedrals` (entries as in calc_dihedral_distribution; the quadruples of
    an entry are pooled into one function) at the lags 0 .. max_lag frames (default (F - 1) // 2); dt: timestep in fs.
    Returns a DataFrame `Time (ps)` and, per entry,
      `C_<label>`  = < cos(phi(t + k) - phi(t)) > over the entry's quadruples, molecules and time origins, and
      `Cn_<label>` = (C - p) / (1 - p) with p = <cos phi>^2 + <sin phi>^2, the plateau C decays to when the distribution
                     is not uniform: Cn goes from 1 to 0 (NaN where p == 1: a torsion that never moves).
    A quadruple with three collinear atoms has no angle: ValueError naming the entries and their counts. With save_mode
    the table is written to dihedral_correlation.csv in working_dir (default: the current directory).
    """
    entries, num_mols, per = _prepare(dihedrals, filename, num_mols, num_atoms_per_mol, coords)
    refuse_triclinic(filename)
    U, times, group_off, degenerate = _load_series(entries, filename, num_mols, per, dt, coords)
    _refuse_degenerate(entries, degenerate)
    max_lag, sums = mol_series.orient_corr(U, group_off, max_lag)
    cols = {"Time (ps)": times[: max_lag + 1] - times[0]}
    origins = (len(times) - np.arange(max_lag + 1)).astype(np.float64)
    for g, (_, _, label) in enumerate(entries):
        lo, hi = int(group_off[g]), int(group_off[g + 1])
        w = origins * float(hi - lo)
        with np.errstate(invalid="ignore", divide="ignore"):
            c = sums[:, g, 0] / w
            mc, ms = (float(U[lo:hi, k].mean()) for k in (0, 1)) if hi > lo else (np.nan, np.nan)
            p = mc * mc + ms * ms
            cols["C_" + label] = c
            cols["Cn_" + label] = (c - p) / (1.0 - p) if p != 1.0 else np.full(len(c), np.nan)
    df = pd.DataFrame(cols)
    if save_mode and is_writer():
        df.to_csv((working_dir or os.getcwd()) + "/dihedral_correlation.csv")
    return df
