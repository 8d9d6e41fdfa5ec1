"""Records the yardstick's results of the colour-balance scenes (tests/color_balance_fixtures.py) under
tests/golden/color_balance/: the oracle's Ceres restatement driven by tests/color_balance_oracle_driver.cpp.  Results
only - summary, message, iteration records, parameters, and the checksum of the scene they belong to; the scenes are
regenerated from their seeds.  A scene one of whose termination decisions sits within a factor 4 of its threshold is
refused.  Run from the repository root: python scripts/make_color_balance_golden.py"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import color_balance_fixtures as F  # noqa: E402


def main():
    os.makedirs(F.GOLDEN, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = F.build_driver(tmp)
        for name, corr in {**F.solve_cases(), "grid20x20": F.grid_case()}.items():
            y = F.run_driver(exe, corr, tmp, name)
            near = F.thresholds_clear(y)
            if near or not y["success"]:
                raise SystemExit(f"{name}: not usable as a fixture: {near}")
            with open(os.path.join(F.GOLDEN, name + ".json"), "w") as f:
                json.dump(y, f, indent=0, sort_keys=True)
            print(name, len(corr), "correspondences,", y["num_iterations"], "iterations,", y["message"])


if __name__ == "__main__":
    main()
