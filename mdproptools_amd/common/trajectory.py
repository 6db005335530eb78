"""
Trajectory ingest shared by the drop-in modules: which route can serve a request, which columns to read, and the
frames themselves — as host batches (`frame_batches`, the native reader) or as page-locked batches from the frame
stream (`stream_reduced`, mdproptools_amd/stream.py). A new drop-in gets its frames from here.
"""

import numpy as np

from .. import io as mio

UNWRAPPED = ("xu", "yu", "zu")
WRAPPED = ("x", "y", "z", "ix", "iy", "iz")


def streamable_files(pattern, needed, files=None):
    """The sorted files of `pattern` (or `files`, a rank's share) when the frame stream can serve the request: at least
    one file, plain text only, and every column of `needed` in the first frame of the first file. None otherwise — for
    a missing column too: the general route names it in the caller's own words."""
    mine = files if files is not None else mio._sorted_matches(pattern)
    if not mine or any(str(f).endswith(".gz") for f in mine):
        return None
    nd = mio.NativeDumpFile(mine[0])
    try:
        names = nd.header(0)[4] if nd.n_frames else []
    finally:
        nd.close()
    return mine if set(needed) <= set(names) else None


def frame_refs(pattern):
    """(file, frame within the file) of every frame, in parse_lammps_dumps order."""
    refs = []
    for fname in mio._sorted_matches(pattern):
        if str(fname).endswith(".gz"):
            n = sum(1 for _ in mio._iter_frames(fname))
        else:
            nd = mio.NativeDumpFile(fname)
            n = nd.n_frames
            nd.close()
        refs += [(fname, k) for k in range(n)]
    return refs


def read_frame(fname, k, columns):
    """(timestep, bounds [3,2], column names, planes [C, N] of `columns` sorted by id) of frame k of one file."""
    if str(fname).endswith(".gz"):
        ts, bounds, _, names, planes = mio._pandas_file_frames(fname, columns, "id")[k]
        return ts, bounds, names, planes
    nd = mio.NativeDumpFile(fname)
    try:
        ts, _, bounds, _, names = nd.header(k)
        return ts, bounds, names, nd.read(k, columns, sort_by="id")
    finally:
        nd.close()


def unwrapped_columns(names, extra, missing, decide_on=UNWRAPPED):
    """The columns to read for unwrapped coordinates: extra + [xu, yu, zu] when every column of `decide_on` is among
    `names`, else extra + [x, y, z, ix, iy, iz] (for `unwrap`). `missing(column, have_unwrapped)` is called for each
    selected column the dump lacks: the caller raises there, in its own words, or returns and leaves it to the reader."""
    have = all(c in names for c in decide_on)
    sel = UNWRAPPED if have else WRAPPED
    for c in sel:
        if c not in names:
            missing(c, have)
    return list(extra) + list(sel)


def unwrap(cols, bounds):
    """Fills xu, yu, zu of the column dict from x + ix * (hi - lo) when zu is absent."""
    if "zu" not in cols:
        for k, axis in enumerate("xyz"):
            cols[axis + "u"] = cols[axis] + cols["i" + axis] * (bounds[k][1] - bounds[k][0])
    return cols


def masses(second_column, mass):
    """Per-atom masses: `second_column` itself (the dump's mass column) without `mass`, else the `mass` list indexed by
    the 1-based types in it."""
    if not mass:
        return second_column
    return np.asarray(mass, dtype=np.float64)[second_column.astype(np.int64) - 1]


def same_labels(labels_per_frame):
    """[N] when every frame carries the same labels, else [F, N]."""
    first = labels_per_frame[0]
    if all(np.array_equal(first, lab) for lab in labels_per_frame[1:]):
        return first
    return np.stack(labels_per_frame)


def frame_batches(pattern, columns, max_bytes, n_atoms=None, files=None):
    """Batches of whole frames in parse_lammps_dumps order, atoms by id: (timesteps, box lengths [B,3], planes [B,C,N]
    of `columns`). A batch holds frames of one atom count and is cut before the frame that would take `planes` past
    `max_bytes` (it holds at least one). Every kernel behind a batch works per frame, so where the cuts fall shows in no
    result. `n_atoms`: the layout's atom count, checked on every frame (check_atom_count)."""
    from .com_mols import check_atom_count

    steps, boxes, planes = [], [], []
    for ts, bounds, _, _, pl in mio.iter_native_frames(pattern, columns, sort_by="id", files=files):
        if n_atoms is not None:
            check_atom_count(n_atoms, pl.shape[1])
        if planes and (pl.shape != planes[0].shape or (len(planes) + 1) * pl.nbytes > max_bytes):
            yield steps, np.stack(boxes), np.stack(planes)
            steps, boxes, planes = [], [], []
        b = np.asarray(bounds, dtype=np.float64)
        steps.append(int(ts))
        boxes.append(b[:, 1] - b[:, 0])
        planes.append(pl)
    if planes:
        yield steps, np.stack(boxes), np.stack(planes)


def stream_reduced(pattern, files, columns, n_atoms_expected, batch_bytes=None):
    """The batches of a `stream.FrameStream` over `files` (from `streamable_files`) with `columns` = (first, second,
    three planes): batch.ids / batch.types [B,N] hold the first two, batch.xyz [B,3,N] the planes, page-locked. Every
    batch is checked against `n_atoms_expected` (None: not checked). What a caller keeps from a batch must be a copy:
    its buffer goes back to the producer when the next one is asked for."""
    from ..stream import FrameStream
    from .com_mols import check_atom_count

    for batch in FrameStream(pattern, files=files, columns=columns, batch_bytes=batch_bytes):
        if n_atoms_expected is not None:
            check_atom_count(n_atoms_expected, batch.xyz.shape[2])
        yield batch
