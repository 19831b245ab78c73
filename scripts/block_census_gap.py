"""Which block kernels a suite run never launched.

  RTX_DEBUG_LAUNCH=1 python -m pytest tests -m gpu --deselect tests/test_block_census.py -s 2> suite.err
  python scripts/block_census_gap.py suite.err [profiles/block_census.json]

Reads the "rtx launch: <name>" lines of the run's stderr (a `sort | uniq -c` of them works too), prints the kernels of
tests/block_kernels.txt that are not among them, and writes them into the record under "not_launched_before"."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    with open(os.path.join(ROOT, "tests", "block_kernels.txt")) as f:
        rows = [ln.split("\t") for ln in f.read().splitlines() if ln and not ln.startswith("#")]
    launched = set()
    with open(argv[1], errors="replace") as f:
        for ln in f:
            if "rtx launch: " in ln:
                launched.add(ln.split("rtx launch: ", 1)[1].strip())
    never = [(m, d) for m, d in rows if m not in launched]
    print(f"{len(rows)} block kernels listed, {len(rows) - len(never)} launched, {len(never)} never:")
    for _, d in never:
        print("  " + d)
    if len(argv) > 2:
        record = {}
        if os.path.exists(argv[2]):
            with open(argv[2]) as f:
                record = json.load(f)
        record["not_launched_before"] = [d for _, d in never]
        with open(argv[2], "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv)
