"""The launches of one step of a rocprofv3 kernel trace (rocpd SQLite), in issue order: kernel name, grid, workgroup, LDS bytes.
    python scripts/trace_launch_list.py kt_results.db > list.txt            one step (see one_step)
    python scripts/trace_launch_list.py a_results.db --same-as b_results.db   exit 1 unless the WHOLE runs launch the same things in the same order
Trace a single-stream run (MOREC_WGRAD_STREAM=0): with two streams the order of starts is not fixed."""
import sqlite3
import sys


def launches(path):
    db = sqlite3.connect(path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)").fetchall()]
    want = [c for c in cols if any(k in c.lower() for k in ("grid", "workgroup", "lds"))]
    rows = db.execute(f"select name, {', '.join(want)} from kernels order by start").fetchall()
    return want, [tuple(r) for r in rows]


def one_step(rows):
    """The launches between two consecutive occurrences of a step marker: the launch that recurs (>= 3 times) with the longest shortest
    distance between occurrences.  Of those stretches the last that equals the one before it, else (token counts, and with them grids,
    change from batch to batch) the last one."""
    where = {}
    for i, r in enumerate(rows):
        where.setdefault(r, []).append(i)
    pos = max((p for p in where.values() if len(p) >= 3), key=lambda p: (min(b - a for a, b in zip(p, p[1:])), -len(p)))
    segs = [rows[a:b] for a, b in zip(pos, pos[1:])]
    for k in range(len(segs) - 1, 0, -1):
        if segs[k] == segs[k - 1]:
            return segs[k]
    return segs[-1]


if __name__ == "__main__":
    want, rows = launches(sys.argv[1])
    if len(sys.argv) > 3 and sys.argv[2] == "--same-as":
        _, other = launches(sys.argv[3])
        same = rows == other
        first = next((i for i, (a, b) in enumerate(zip(rows, other)) if a != b), min(len(rows), len(other)))
        print(f"{len(rows)} vs {len(other)} launches: " + ("identical (name, " + ", ".join(want) + ") in the same order" if same else f"DIFFER from launch {first}: {rows[first:first + 1]} vs {other[first:first + 1]}"))
        sys.exit(0 if same else 1)
    step = one_step(rows)
    print(f"# {len(step)} launches per step ({len(rows)} in the run); columns: name, " + ", ".join(want))
    for r in step:
        print("\t".join(str(x) for x in r))
