#!/usr/bin/env python3
"""Record what the moment-statistics entry points return on the fixed inputs of
tests/moment_stats.py (hashes of the maps, lists, canvases and denoised
moments, the summaries as hex floats) into tests/golden/moment_stats_parent.json.

The file was recorded from the library of the commit before csrc/host/moments.h
(RTW_LIBRARY=<that build's librtw.so>; the ABI is the same, so this tree's
Python drives it): the host half on a CPU, the device half (--device) on an
MI355X.  tests/test_moment_stats.py compares the library now with it.

  RTW_LIBRARY=... python scripts/record_moment_stats.py [--device] [--out FILE]

Writes the half it ran and keeps the other half of FILE."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

if __name__ == "__main__":
    import moment_stats
    from raytracingweekend_amd import render

    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--out", type=Path, default=moment_stats.GOLDEN)
    args = ap.parse_args()
    doc = json.loads(args.out.read_text()) if args.out.exists() else {}
    doc["device" if args.device else "host"] = moment_stats.record(render, args.device)
    args.out.write_text(json.dumps(doc, indent=1, sort_keys=True) + "\n")
    print(f"wrote {args.out} ({', '.join(sorted(doc))})")
