"""Record tests/golden/abi_refusals.json: the (status, message) of every refused
C-ABI call in tests/abi_refusal_cases.py, which tests/test_abi_refusals_cpu.py
replays.  Needs a built library and no GPU.  Runs the table twice and refuses
to write unless both runs agree and every call was refused by an argument
check.  A case that is already in the file keeps its "old_message" (the text
before a deliberate change).

    python scripts/record_abi_refusals.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import abi_refusal_cases  # noqa: E402
from cnn_graph_amd import _lib  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "abi_refusals.json")
    first, second = abi_refusal_cases.run(), abi_refusal_cases.run()
    if first != second:
        sys.exit(f"two recordings differ in {[k for k in first if first[k] != second[k]]}")
    loose = [k for k, v in first.items() if v["status"] not in (_lib.CG_ERR_ARG, _lib.CG_ERR_UNSUPPORTED)]
    if loose:
        sys.exit(f"not refused by an argument check: {loose}")
    if os.path.exists(out):
        with open(out) as f:
            old = json.load(f)
        for k, v in first.items():
            before = old.get(k, {}).get("old_message", old.get(k, {}).get("message"))
            if before is not None and before != v["message"]:
                v["old_message"] = before
    with open(out, "w") as f:  # one line per case
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(first[k], sort_keys=True)}"
                                   for k in sorted(first)) + "\n}\n")
    print(f"{len(first)} refusals, two recordings identical -> {out}")


if __name__ == "__main__":
    main()
