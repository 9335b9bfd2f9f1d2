"""Turn hipcc's -Rpass-analysis=kernel-resource-usage remarks (stderr of a
compile, read from stdin) into one line per kernel: registers, scratch,
occupancy, static LDS.

  hipcc --offload-arch=gfx950 <flags of the Makefile> -Rpass-analysis=kernel-resource-usage \
      -c csrc/ldt_resize4.hip -o /dev/null 2>&1 | python tools/resource_table.py

k_resize4 instantiations are named k_resize4<SRC,KS[,gen]>; other kernels keep
their mangled names."""
import re
import sys

KEYS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill",
        "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def short(name: str) -> str:
    m = re.search(r"k_resize4ILi(\d+)ELi(\d+)(?:ELb(\d))?", name)
    if not m:
        return name
    return "k_resize4<%s,%s%s>" % (m.group(1), m.group(2), ",gen" if m.group(3) == "1" else "")


def main() -> None:
    rows, cur = {}, None
    for line in sys.stdin:
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(short(m.group(1)), {})
            continue
        m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    print("kernel | " + " | ".join(KEYS))
    for name in sorted(rows):
        print(name + " | " + " | ".join(rows[name].get(k, "?") for k in KEYS))


if __name__ == "__main__":
    main()
