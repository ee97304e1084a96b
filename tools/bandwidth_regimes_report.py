#!/usr/bin/env python3
"""Writes profiles/r9_bandwidth_regimes.json: the records of tests/test_bandwidth_regimes.py (one per case: predicate
values, eigenvalue error, the elementwise excess over one fp32 ulp per layer and per named region, whole-plane relative
L2, the differences between kernel forms), with their maxima.  The test's constants A_REL and L2_REL are ten times these
maxima.  Needs an MI355X.

    python tools/bandwidth_regimes_report.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_bandwidth_regimes as tb  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else tb.PROFILE
    cases = {}
    for case, cid in zip(tb.CASES, tb.CASE_IDS):
        s, rec = tb.setup(case), tb.record(case)
        cases[cid] = dict(rec, lam_min_Ka=s["lam_min"], min_row_sum=s["min_row_sum"], hx=s["hx"], planes=tb.planes(s))
        print(cid, "eig %.1e" % rec["eig_err"], "excess %.2e" % max(max(v) for v in rec["excess"].values()),
              "rel L2 %.2e" % max(rec["rel_l2"]), "forced plain: bitwise", rec["forced_plain"]["bitwise"], flush=True)
    doc = dict(what="tests/test_bandwidth_regimes.py on one MI355X: device (default settings) against the fp64 oracle; "
                    "excess = max over pixels of (|Y - Y_o| - 2^-23 |Y_o|) / max|Y_o[j]|, floored at 0, per plane "
                    "(the layers, then apply with weights %s)" % tb.APPLY_WEIGHTS,
               max_excess=max(max(max(v) for v in c["excess"].values()) for c in cases.values()),
               max_rel_l2=max(max(c["rel_l2"]) for c in cases.values()),
               max_eig_err=max(c["eig_err"] for c in cases.values()),
               cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("max excess %.3e  max rel L2 %.3e  max eig err %.3e -> %s" % (doc["max_excess"], doc["max_rel_l2"],
                                                                      doc["max_eig_err"], out))
    over = [cid for cid, c in cases.items() if max(max(v) for v in c["excess"].values()) > tb.FINDING]
    print("cases with an excess above %.0e (each one a finding to explain):" % tb.FINDING, over or "none")


if __name__ == "__main__":
    main()
