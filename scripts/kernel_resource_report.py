"""One line per kernel from the -Rpass-analysis=kernel-resource-usage remarks of
a build log (`make EXTRA=-Rpass-analysis=kernel-resource-usage 2> log`), sorted,
so that the reports of two builds can be compared with cmp / diff:

    location  mangled name  SGPRs VGPRs AGPRs scratch dyn-stack occupancy sgpr-spill vgpr-spill LDS

    python scripts/kernel_resource_report.py build.log > report.txt
"""
import re
import sys

KEYS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Dynamic Stack",
        "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")
REMARK = re.compile(r"^(.*?:\d+:\d+): remark: +([^:]+): (.*?) \[-Rpass")


def main():
    rows, cur = [], None
    for line in open(sys.argv[1]):
        m = REMARK.match(line)
        if not m:
            continue
        loc, key, value = m.groups()
        if key == "Function Name":
            cur = (loc, value, {})
            rows.append(cur)
        elif cur is None or cur[0] != loc or key in cur[2]:
            sys.exit(f"remarks of two kernels are interleaved at: {line.strip()}")
        else:
            cur[2][key] = value
    for loc, name, v in sorted(rows, key=lambda r: (r[0], r[1], sorted(r[2].items()))):
        print(loc, name, *(v[k] for k in KEYS))


if __name__ == "__main__":
    main()
