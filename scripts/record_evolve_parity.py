#!/usr/bin/env python3
"""Record tests/golden/evolve_parity.json: the sha256 of every array the parity cases of
tests/test_device_evolve_host.py compare, taken from libmtgp_host.so, after checking that the host
twin of libmtgp_hip.so hashes to the same values.

Run once, on the last commit that had two C++ implementations of the evolution step (the libraries
built from that commit, the case list of this one): the file is what both drivers of the single
implementation are held against afterwards.  Running it on a later commit would only record the
implementation against itself.

    scripts/record_evolve_parity.py <commit the libraries were built from>
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_device_evolve_host as cases  # noqa: E402

commit = sys.argv[1]
out = {"recorded_from": "libmtgp_host.so (mtgp_evolve_populations, mtgp_sample_population); the host twin "
                        "(mtgp_evolve_device_host, mtgp_sample_population_device_host) gave the same digests",
       "commit": commit, "digest": "sha256 of the float32 array's bytes, C order", "cases": {}}
for case in cases.PARITY_CASES:
    d = cases.parity_digests(case)
    assert d["host"] == d["twin"], f"{case}: host library and twin differ"
    out["cases"][case] = d["host"]
    print(case, len(d["host"]), "arrays", flush=True)
with open(cases.GOLDEN, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
