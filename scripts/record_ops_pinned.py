"""Record tests/golden/ops_pinned.json: the refusals (exception type and text)
and output digests of tests/ops_pinned_cases.py, which
tests/test_gpu_ops_pinned.py replays.  Needs the GPU and a built library.  Runs
everything twice and refuses to write unless the two recordings agree.  A
refusal that is already in the file keeps its "old_message" (the text before a
deliberate change).

    python scripts/record_ops_pinned.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import ops_pinned_cases as cases  # noqa: E402


def record(dev):
    return {"refusals": cases.refused(dev), "abi_refusals": cases.abi_refused(dev),
            "results": cases.results(dev)}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ops_pinned.json")
    dev = torch.device("cuda", 0)
    first, second = record(dev), record(dev)
    differ = [(s, k) for s in first for k in first[s] if first[s][k] != second[s][k]]
    if differ:
        sys.exit(f"two recordings differ in {differ}")
    if os.path.exists(out):
        with open(out) as f:
            old = json.load(f)
        for s in ("refusals", "abi_refusals"):
            for k, v in first[s].items():
                o = old.get(s, {}).get(k, {})
                before = o.get("old_message", o.get("message"))
                if before is not None and before != v["message"]:
                    v["old_message"] = before
    with open(out, "w") as f:  # one line per case
        f.write("{\n" + ",\n".join(
            f" {json.dumps(s)}: {{\n" + ",\n".join(
                f"  {json.dumps(k)}: {json.dumps(first[s][k], sort_keys=True)}" for k in sorted(first[s]))
            + "\n }" for s in sorted(first)) + "\n}\n")
    print(f"{len(first['refusals'])} + {len(first['abi_refusals'])} refusals, {len(first['results'])} "
          f"result cases, two recordings identical -> {out}")


if __name__ == "__main__":
    main()
