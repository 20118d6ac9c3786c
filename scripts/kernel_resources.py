"""Register, scratch and LDS use of the fused-pass kernels, from the compiler's
kernel-resource-usage remarks.  Compile the device code of slio_device.hip with
the product flags plus

  --cuda-device-only -Rpass-analysis=kernel-resource-usage -c ... 2> remarks.txt

and give the remark files (one per tree) to this script: one table per file,
one row per fused k_search_pass instantiation and per k_update_persist.

  python scripts/kernel_resources.py before=remarks_a.txt after=remarks_b.txt
"""
import re
import sys

FIELDS = [("VGPRs", "VGPR"), ("AGPRs", "AGPR"), ("TotalSGPRs", "SGPR"), ("ScratchSize [bytes/lane]", "scratch B/lane"),
          ("VGPRs Spill", "VGPR spill"), ("SGPRs Spill", "SGPR spill"), ("LDS Size [bytes/block]", "LDS B"),
          ("Occupancy [waves/SIMD]", "waves/SIMD")]


def label(mangled):
    m = re.match(r"_ZN4slio13k_search_passILi(\d+)ELi(\d+)ELb(\d)ELb(\d)ELb(\d)ELi(\d+)E(?:Lb(\d)E)?EE", mangled)
    if m:
        lpq, u, sph, dev, fuse, d, red = (int(v or 0) for v in m.groups())
        if not fuse:
            return None
        return (f"k_search_pass<{lpq}, {u}, {bool(sph)}, DEVPOSE={bool(dev)}, FUSE, D={d}"
                f"{', RED' if red else ''}>").replace("True", "true").replace("False", "false")
    m = re.match(r"_ZN4slio16k_update_persistILi(\d+)ELi(\d+)EEE", mangled)
    if m:
        return f"k_update_persist<{m.group(1)}, D={m.group(2)}>"
    return None


def parse(path):
    rows, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = label(m.group(1))
            if cur:
                rows[cur] = {}
            continue
        if cur:
            m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass-analysis", line)
            if m:
                rows[cur][m.group(1)] = m.group(2)
    return rows


for arg in sys.argv[1:]:
    name, path = arg.split("=", 1)
    rows = parse(path)
    print(f"### {name}\n")
    print("| kernel | " + " | ".join(h for _, h in FIELDS) + " |")
    print("|---|" + "---|" * len(FIELDS))
    for k in sorted(rows):
        print(f"| `{k}` | " + " | ".join(rows[k].get(f, "?") for f, _ in FIELDS) + " |")
    print()
