"""Record tests/golden/fres_bits.json: the digests tests/test_gpu_fres_bits.py
replays (the cases are tests/fres_bits_cases.py).  Needs the GPU and a built
library.  Runs every case twice and refuses to write unless the two
recordings agree: these kernels have no atomics.

    python scripts/record_fres_bits.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import fres_bits_cases  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "fres_bits.json")
    dev = torch.device("cuda", 0)
    first, second = fres_bits_cases.run(dev), fres_bits_cases.run(dev)
    differ = [k for k in first if first[k] != second[k]]
    if differ:
        sys.exit(f"two recordings differ in {differ}")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(first, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(first)} cases, two recordings identical -> {out}")


if __name__ == "__main__":
    main()
