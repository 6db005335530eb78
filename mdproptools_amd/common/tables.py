"""
What the drop-in modules share on the way from integer counts to the tables they return and write.
"""

import numpy as np


def density(counts, width):
    """counts / (total * width): integrates to 1; all NaN without counts."""
    counts = np.asarray(counts).astype(np.int64)
    total = int(counts.sum())
    return counts / (total * width) if total else np.full(len(counts), np.nan)


def write_csv(df, path_or_buf):
    """`df.to_csv(path_or_buf, index=False)` — byte for byte — for the all-float64 frames these functions write,
    without pandas' per-cell formatting machinery (20 ms for 400 x 12 values, a quarter of a C2-size call): pandas
    writes the shortest round-trip decimal of every double, which is Python's repr, and an empty field for NaN."""
    simple = (isinstance(path_or_buf, (str, bytes)) or hasattr(path_or_buf, "__fspath__")) and \
        all(str(t) == "float64" for t in df.dtypes) and \
        not any(ch in str(c) for c in df.columns for ch in ',"\n\r')
    if not simple:
        df.to_csv(path_or_buf, index=False)
        return
    lines = [",".join(str(c) for c in df.columns)]
    for row in df.to_numpy().tolist():
        lines.append(",".join("" if v != v else repr(v) for v in row))
    with open(path_or_buf, "w", newline="") as fh:
        fh.write("\n".join(lines) + "\n")
