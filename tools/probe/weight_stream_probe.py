#!/usr/bin/env python3
"""weight_stream_probe.py — driver of weight_stream_probe.hip (see there): builds the program if it is not there, runs it
under a time limit, keeps its JSON lines (one per round and arm) and prints, per shape, every arm's median rate, its
round-to-round spread and its distance from the shape's `gemm` arm in units of that arm's spread.

  python tools/probe/weight_stream_probe.py --out profiles/weight_stream_pattern_probe.jsonl
  python tools/probe/weight_stream_probe.py --table profiles/weight_stream_pattern_probe.jsonl   # the table only, no GPU
"""
import argparse, json, os, statistics, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "weight_stream_probe.hip")
EXE = os.path.join(HERE, "weight_stream_probe")


def build():
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Xclang", "-target-feature", "-Xclang",
           "-packed-fp32-ops", SRC, "-o", EXE]
    subprocess.run(cmd, check=True)


def table(rows):
    lines = ["| shape | arm | streams | pad | KiB in flight / wave | grid | barrier | µs (median) | TB/s (median) | "
             "spread TB/s | vs `gemm`, in `gemm` spreads |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    by = {}
    for r in rows:
        by.setdefault((r["shape"], r["arm"]), []).append(r)
    base = {}
    for (shape, arm), rs in by.items():
        if arm == "gemm":
            t = [r["TBps"] for r in rs]
            base[shape] = (statistics.median(t), max(t) - min(t))
    for (shape, arm), rs in by.items():
        t = [r["TBps"] for r in rs]
        med, spread = statistics.median(t), max(t) - min(t)
        b_med, b_spread = base[shape]
        rel = (med - b_med) / b_spread if b_spread > 0 else float("inf") if med != b_med else 0.0
        r = rs[0]
        lines.append(f"| {shape} | {arm} | {r['streams']}{'/spread' if r.get('spread') else ''} x{r['waves']} | {r['pad']} | {r['flight_KiB']} | "
                     f"{r['grid'][0]}x{r['grid'][1]} | {'yes' if r['sync'] else 'no'} | "
                     f"{statistics.median(x['us'] for x in rs):.2f} | {med:.3f} | {spread:.3f} | {rel:+.1f} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="where the JSON lines go (default: stdout only)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=256)
    ap.add_argument("--timeout", type=float, default=60.0, help="seconds; the GPU work itself is about one second")
    ap.add_argument("--table", default=None, help="print the table of an earlier run's JSON lines and exit")
    a = ap.parse_args()
    if a.table:
        with open(a.table) as f:
            print(table([json.loads(l) for l in f if l.strip()]))
        return 0
    if not os.path.exists(EXE):
        build()
    p = subprocess.run([EXE, "--rounds", str(a.rounds), "--launches", str(a.launches)], stdout=subprocess.PIPE,
                       text=True, timeout=a.timeout)
    if p.returncode != 0:
        print(p.stdout, end="")
        print(f"weight_stream_probe ended with status {p.returncode}", file=sys.stderr)
        return p.returncode
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.strip()]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(p.stdout)
    print(p.stdout, end="")
    print(table(rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
