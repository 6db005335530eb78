"""
Trajectory ingest shared by the drop-in modules: which route can serve a request, which columns to read, and the
frames themselves — as host batches (`frame_batches`, the native reader), as host batches of x y z under one set of
atom types (`typed_batches`: the structural analyses), as page-locked batches from the frame stream (`stream_reduced`,
mdproptools_amd/stream.py), as two per-atom attributes and three planes from whichever of the two can serve
(`attribute_batches`: the dynamical drop-ins), or as whole id-sorted frames batched for the pair loops (`load_frames`,
`batches`, `all_frames`). `refuse_triclinic` is the box rule of every analysis that takes orthogonal boxes only. A new
drop-in gets its frames from here.
"""

import numpy as np

from .. import io as mio

UNWRAPPED = ("xu", "yu", "zu")
WRAPPED = ("x", "y", "z", "ix", "iy", "iz")
TYPED_BATCH_BYTES = 1 << 28  # planes of the frames that typed_batches hands over for one library call
SAME_TYPES = "every frame must hold the same atom types in id order"


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


def refuse_triclinic(pattern):
    """ValueError when the first frame of a plain-text file of `pattern` has a triclinic box (.gz files are not looked
    into)."""
    for fname in mio._sorted_matches(pattern):
        if str(fname).endswith(".gz"):
            continue
        nd = mio.NativeDumpFile(fname)
        try:
            if nd.n_frames and nd.header(0)[3] is not None:
                raise ValueError("triclinic boxes are not supported")
        finally:
            nd.close()


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


def typed_batches(pattern, num_mols, num_atoms_per_mol, altered, max_bytes=None, mismatch=SAME_TYPES):
    """`frame_batches` of id type x y z for the analyses that run under ONE set of atom types: (timesteps, box lengths
    [B,3], xyz [B,3,N] C-contiguous float64, types int32 [N]). `types` are the labels of the first frame — with
    `altered` calc_atom_type of its ids, else its `type` column — and the same array in every batch; a later frame
    whose labels differ in length or value raises ValueError(`mismatch`). With both layout arguments every frame is
    checked against the layout's atom count. `max_bytes` None: TYPED_BATCH_BYTES, read when the loop starts."""
    from .com_mols import calc_atom_type, molecule_layout

    n_atoms = None
    if num_mols is not None and num_atoms_per_mol is not None:
        n_atoms = int(molecule_layout(num_mols, num_atoms_per_mol)[0][-1])
    cap = TYPED_BATCH_BYTES if max_bytes is None else max_bytes
    types = None
    for steps, boxes, planes in frame_batches(pattern, ["id", "type", "x", "y", "z"], cap, n_atoms):
        for pl in planes:
            lab = calc_atom_type(pl[0], num_mols, num_atoms_per_mol) if altered else pl[1]
            if types is None:
                types = lab.astype(np.int32)
            elif len(lab) != len(types) or not np.array_equal(lab, types):
                raise ValueError(mismatch)
        yield steps, boxes, np.ascontiguousarray(planes[:, 2:5]), types


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


def _keep_row(rows, row):
    """Appends the per-atom row [N] of one frame to `rows`: the first frame's array itself where the frame repeats it
    (attributes seldom change, and then nothing is held twice), else a copy."""
    rows.append(rows[0] if rows and np.array_equal(rows[0], row) else row.copy())


def attribute_batches(pattern, leading, planes, n_atoms=None, files=None, stream=True, batch_bytes=None, missing=None,
                      decide_on=UNWRAPPED, dumps=None, with_box=False):
    """The frames of `pattern` (or of `files`, a rank's share: native reader only) in parse_lammps_dumps order, atoms by
    id, reduced to two `leading` per-atom columns and three `planes` — `UNWRAPPED`, or any three columns such as vx vy
    vz. Returns (streamed, batches): `batches` yields host batches (timesteps [B], first [B,N], second [B,N], planes
    [B,3,N]) whatever route serves them, and `streamed` says, before the first one, which route was chosen:

    the frame stream, when the caller allows it (`stream`), io.USE_NATIVE_READER is set and `streamable_files` accepts
    the files: batches of `batch_bytes` (stream.frames_per_batch) that live in staging buffers — what a caller keeps
    from one must be a copy;

    else the general route — the native reader, or pandas over `dumps` (the caller's own parsed frames; default:
    parse_lammps_dumps(pattern)) — with every frame in ONE batch (nothing when there is no frame), so that a caller
    makes one library call there. It makes xu yu zu from x + ix * L where `decide_on` says the dump has none
    (`unwrapped_columns`, `unwrap`), and hands what the dump lacks to the caller first: `missing([columns], names)`, the
    columns in the order id, leading, planes. The caller raises there in its own words, or returns and leaves it to
    the reader. A per-atom row that every frame repeats is held once there: [B,N] is then a read-only view of it. A
    stream that produced no frame of a whole pattern hands out this route's batch instead.

    `with_box`: every batch carries a fifth entry, the box edge lengths [B,3] (hi - lo of the bounds) of its frames —
    what a caller that reads wrapped coordinates (planes x y z) needs beside them.

    Every frame is checked against `n_atoms` (check_atom_count; None: not checked)."""
    from .com_mols import check_atom_count

    leading, planes = list(leading), list(planes)
    unwrapped = planes == list(UNWRAPPED)
    mine = streamable_files(pattern, ["id"] + leading + planes, files) if stream and mio.USE_NATIVE_READER else None

    def wanted(names):  # (the reader's own error names the first column of this list that the dump lacks)
        sel = unwrapped_columns(names, leading, lambda c, have: None, decide_on) if unwrapped else planes + leading
        sel = list(dict.fromkeys(sel))  # (a column named twice is read once)
        lacking = [c for c in dict.fromkeys(["id"] + leading + sel) if c not in names]
        if lacking and missing is not None:
            missing(lacking, names)
        return sel

    def parsed():
        for dump in dumps if dumps is not None else mio.parse_lammps_dumps(pattern):
            sel = wanted(list(dump.data.columns))
            data = dump.data.sort_values(by=["id"])
            yield dump.timestep, dump.box.bounds, {c: data[c].to_numpy(dtype=np.float64) for c in sel}

    def batches():
        if mine is not None:
            served = False
            for b in stream_reduced(pattern, mine, leading + planes, n_atoms, batch_bytes):
                served = True
                yield (b.timesteps, b.ids, b.types, b.xyz) + ((np.asarray(b.lengths, dtype=np.float64),) if with_box else ())
            if served or files is not None:
                return
        frames = parsed()
        if mio.USE_NATIVE_READER:
            frames = ((ts, bounds, dict(zip(wanted(names), pl))) for ts, bounds, _l, names, pl in
                      mio.iter_native_frames(pattern, wanted, sort_by="id", files=files))
        steps, xyz, boxes, rows = [], [], [], {c: [] for c in leading}
        for ts, bounds, cols in frames:
            if unwrapped:
                unwrap(cols, bounds)
            if n_atoms is not None:
                check_atom_count(n_atoms, len(cols[planes[0]]))
            steps.append(int(ts))
            if with_box:
                b = np.asarray(bounds, dtype=np.float64)
                boxes.append(b[:, 1] - b[:, 0])
            xyz.append(np.stack([cols[c] for c in planes]))
            for c in rows:
                _keep_row(rows[c], cols[c])
        if steps:
            held = {c: np.broadcast_to(r[0], (len(r), len(r[0]))) if all(x is r[0] for x in r) else np.stack(r)
                    for c, r in rows.items()}
            yield (np.array(steps, dtype=np.int64), held[leading[0]], held[leading[1]], np.stack(xyz)) + (
                (np.stack(boxes),) if with_box else ())

    return mine is not None, batches()


# ------------------------------------------------------------------------------------------------
# whole frames for the pair loops: id-sorted SoA planes, batched for one library call each
# ------------------------------------------------------------------------------------------------


class Frame:
    """One parsed frame reduced to what the pair loops need (rdf_cn.py:183-194): id-sorted ids, types,
    xyz planes [3,N] and the box edge lengths."""

    __slots__ = ("timestep", "ids", "types", "xyz", "lengths")

    def __init__(self, timestep, ids, types, xyz, lengths):
        self.timestep, self.ids, self.types, self.xyz, self.lengths = timestep, ids, types, xyz, lengths

    @classmethod
    def from_dump(cls, dump):
        tbl = dump.data[["id", "type", "x", "y", "z"]].sort_values("id").to_numpy(dtype=np.float64)
        return cls(dump.timestep, tbl[:, 0], tbl[:, 1], np.ascontiguousarray(tbl[:, 2:5].T),
                   dump.box.to_lattice().lengths)


def load_frames(filename, shard=False, stream=False, on_frame=None):
    """Every frame of `filename` (file or '*' pattern, numeric order). The native reader of libmdhip.so
    produces the same doubles as the pandas-based one (tests/test_dump_reader_cpu.py), ~10x faster.
    `on_frame(timestep)` is called as each frame is parsed (the caller's progress line).

    stream=True (what the public functions ask for): a `stream.FrameStream` instead of a list — `batches` then
    yields batches as the producer thread finishes parsing them, the frames of the trajectory are never all
    resident on the host (the reference builds the whole list first, rdf_cn.py:176).

    shard=True under torch.distributed (one process per GPU): a rank parses and returns only ITS share of the
    trajectory — a contiguous block of the files when there are at least as many files as ranks, else a
    contiguous block of the frames — so that parsing, the usual bottleneck, scales with the ranks too."""
    from .. import dist as D

    def parsed(frame):
        if on_frame is not None:
            on_frame(frame.timestep)
        return frame

    sharded = shard and D.is_distributed()
    files = None
    if sharded and (isinstance(filename, str) or hasattr(filename, "__fspath__")):
        matches = mio._sorted_matches(str(filename))
        if len(matches) >= D.rank_world()[1]:
            files = D.shard_items(matches)
    is_path = isinstance(filename, str) or hasattr(filename, "__fspath__")
    if stream and mio.USE_NATIVE_READER and is_path and (not sharded or files is not None):
        from ..stream import FrameStream

        return FrameStream(str(filename), files=files, on_frame=on_frame)
    if mio.USE_NATIVE_READER and is_path:
        frames = [parsed(Frame(ts, planes[0], planes[1], np.ascontiguousarray(planes[2:5]), lengths))
                  for ts, _b, lengths, _names, planes in
                  mio.iter_native_frames(str(filename), ["id", "type", "x", "y", "z"], sort_by="id", files=files)]
    elif files is not None:
        frames = [parsed(Frame.from_dump(d)) for fn in files for d in mio.parse_lammps_dumps(fn)]
    else:
        frames = [parsed(Frame.from_dump(d)) for d in mio.parse_lammps_dumps(filename)]
    if sharded and files is None:
        frames = D.shard_items(frames)
    return frames


def load_typed_positions(filename, atom_types, coords, dt_ps, what="a displacement"):
    """What Displacement and StructuralRelaxation hand the library: (r [F,3,E] the atoms of the requested types, grouped
    by type in the order of atom_types, ids ascending inside a type; box [F,3]; group_off [T+1]; frame spacing in ps).
    coords "wrapped" reads x y z, "unwrapped" xu yu zu; dt_ps: the timestep in ps. Triclinic boxes, frames that do not
    hold the same atoms, fewer than two frames (`what` needs them) and uneven frame spacing raise ValueError."""
    xyz_cols = ["x", "y", "z"] if coords == "wrapped" else ["xu", "yu", "zu"]
    steps, boxes, planes = [], [], []
    ids = types = sel = None
    for ts, bounds, lengths, _, pl in mio.iter_native_frames(filename, ["id", "type"] + xyz_cols, sort_by="id"):
        b = np.asarray(bounds, dtype=np.float64)
        ext = b[:, 1] - b[:, 0]
        if np.any(np.abs(np.asarray(lengths, dtype=np.float64) - ext) > 1e-12 * np.abs(ext)):
            raise ValueError("triclinic boxes are not supported")
        if ids is None:
            ids, types = pl[0].copy(), pl[1].copy()
            groups = [np.flatnonzero(types == t) for t in atom_types]
            group_off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
            sel = np.concatenate(groups).astype(np.int64) if groups else np.zeros(0, dtype=np.int64)
        elif pl.shape[1] != len(ids) or not np.array_equal(pl[0], ids) or not np.array_equal(pl[1], types):
            raise ValueError("every frame must hold the same atom ids with the same types")
        steps.append(int(ts))
        boxes.append(ext)
        planes.append(pl[2:5][:, sel])
    if len(steps) < 2:
        raise ValueError("%s needs at least two frames" % what)
    d_step = np.diff(np.asarray(steps, dtype=np.int64))
    if d_step[0] <= 0 or np.any(d_step != d_step[0]):
        raise ValueError("the frames must be uniformly spaced in time")
    r = np.ascontiguousarray(np.stack(planes), dtype=np.float64)
    return r, np.ascontiguousarray(np.stack(boxes)), group_off, float(d_step[0]) * dt_ps


def all_frames(per_frame_rows):
    """Per-frame result rows of every rank in frame order (identity without torch.distributed). Ranks hold
    contiguous blocks of the trajectory, so the concatenation in rank order is the frame order, and summing
    the gathered rows in that order gives bit for bit what one process gets."""
    from .. import dist as D

    if len(per_frame_rows) and np.ndim(per_frame_rows[0]) == 2:  # per-batch blocks [B, W]
        rows = np.concatenate(per_frame_rows)
    else:
        rows = np.stack(per_frame_rows) if len(per_frame_rows) else None
    if not D.is_distributed():
        return [] if rows is None else rows
    # Fewer frames than ranks: the ranks without a frame contribute no rows (round 6; they used to make every rank raise).
    # The row width of an empty rank comes from the others, with the counts, in one small all-gather.
    mine = (0, 0) if rows is None else (int(rows.shape[0]), int(rows.shape[1]))
    both = D.allgather_var(np.array([mine], dtype=np.int64), counts=[1] * D.rank_world()[1])
    counts, width = [int(c) for c in both[:, 0]], int(both[:, 1].max())
    if sum(counts) == 0:
        return []
    if rows is None:
        rows = np.zeros((0, width))
    return D.allgather_var(rows, counts=counts)


class Batch(list):
    """The frames of one library call; `block` = their coordinates as ONE array [B,3,N] when they already sit in a
    staging buffer (streamed batches), else None."""

    block = None
    uniform_types = False
    types_ref = None
    lengths_block = None


def lengths_block(batch):
    lb = getattr(batch, "lengths_block", None)
    return lb if lb is not None else np.array([f.lengths for f in batch])


def xyz_block(batch):
    return batch.block if getattr(batch, "block", None) is not None else np.stack([f.xyz for f in batch])


def batches(frames, max_bytes):
    """Consecutive frames with the same atom count, capped at `max_bytes` of coordinates. A FrameStream
    yields its own batches (the staging buffer goes back to the producer when the loop asks for the next one:
    everything a caller keeps from a batch must be a copy)."""
    if not isinstance(frames, list):
        for sb in frames:
            b = Batch(Frame(fr.timestep, fr.ids, fr.types, fr.xyz, fr.lengths) for fr in sb)  # views into the buffer
            b.block = sb.xyz
            b.uniform_types, b.types_ref = getattr(sb, "uniform_types", False), getattr(sb, "types_ref", None)
            b.lengths_block = np.asarray(sb.lengths, dtype=np.float64)
            yield b
        return
    start = 0
    while start < len(frames):
        n = frames[start].xyz.shape[1]
        cap = max(1, max_bytes // max(1, 24 * n))
        stop = start + 1
        while stop < len(frames) and stop - start < cap and frames[stop].xyz.shape[1] == n:
            stop += 1
        yield frames[start:stop]
        start = stop
