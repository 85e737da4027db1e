#!/usr/bin/env python3
"""bench.py with test switches of libhgx set for the whole run (a sweep over a measurement switch on one box):
tools/bench_with_switch.py name=value [name=value ...] [bench.py flags].  The switches live in the process (hgx_test_switch_set), so
they are set after the library is loaded and before bench.py's own main() runs; child processes of bench.py do not see them (run
with --no-e2e).  Example, the sweep of DESIGN.md 5.7: tools/bench_with_switch.py gene_slices_verify=8 --no-cpu-baseline --no-e2e
--no-workloads --steps 100 --warmup 10."""
import os, sys, runpy
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hisatgenotype_amd                      # registers the package directory
from hisatgenotype_amd import engine
rest = sys.argv[1:]
while rest and "=" in rest[0] and not rest[0].startswith("-"):
    name, value = rest.pop(0).split("=", 1)
    engine.test_switch(name, value)
sys.argv = [os.path.join(ROOT, "bench.py")] + rest
runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
