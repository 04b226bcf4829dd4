"""Development aid: A/B two builds of the library in one process-per-arm loop on the same box."""
import json, os, subprocess, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
arms = [a for a in sys.argv[1:] if not a.startswith("--") and a not in ("u32", "u64", "f32")]  # library paths
extra = [a for a in sys.argv[1:] if a not in arms]                                              # the rest goes to bench.py (--dtype u64, --no-extras ...)
code = '''
import sys, json
sys.path.insert(0, %r)
from rdst_amd import _lib
_lib.LIB_PATH = %r
import runpy
sys.argv = ["bench.py", "--full", "--no-cpu-baseline", "--steps", "6", "--warmup", "2"] + %r
runpy.run_path(%r, run_name="__main__")
'''
for rep in range(3):
    for lib in arms:
        out = subprocess.run([sys.executable, "-c", code % (root, os.path.join(root, lib), extra, os.path.join(root, "bench.py"))],
                             capture_output=True, text=True)
        if not any(l.startswith("{") for l in out.stdout.splitlines()):
            print(lib, "FAILED:", out.stderr[-600:]); continue
        out = out.stdout
        line = [l for l in out.splitlines() if l.startswith("{")][-1]
        d = json.loads(line)
        print(f"{lib:40s} {d['value']:8.2f} Gkeys/s  pass {d.get('roofline', {}).get('avg_launch_ms', float('nan')):.4f} ms", flush=True)
