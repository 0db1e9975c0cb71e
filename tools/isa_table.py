"""Per-kernel resources of two device-only assemblies of the same source, side by side (no GPU needed):

    hipcc <the product's flags, impop_amd/build.py> --cuda-device-only -S -o old.s impop_amd/csrc/scan.hip   # at the parent
    hipcc ...                                                           -S -o new.s impop_amd/csrc/scan.hip   # at the change
    python tools/isa_table.py old.s new.s

From the .amdhsa metadata: VGPRs, SGPRs, scratch bytes, spilled VGPRs + SGPRs, LDS bytes; from the body: global_load_*
and s_waitcnt vmcnt instructions.  `same` = the kernel's instructions are identical."""
import re
import subprocess
import sys

KEYS = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("scratch", ".private_segment_fixed_size"), ("vspill", ".vgpr_spill_count"),
        ("sspill", ".sgpr_spill_count"), ("lds", ".group_segment_fixed_size"))


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(\w+):.*?\n(.*?)^\s*\.amdhsa_kernel \1$", text, re.S | re.M):
        body = [ln.split(";")[0].strip() for ln in m.group(2).splitlines()]
        body = [ln for ln in body if ln and not ln.startswith(".")]
        out[m.group(1)] = {"body": body, "loads": sum(ln.startswith("global_load_") for ln in body),
                           "waits": sum(ln.startswith("s_waitcnt") and "vmcnt" in ln for ln in body)}
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target)", text, re.S | re.M):
        meta = dict(re.findall(r"^\s+(\.\w+):\s+(\S+)$", m.group(0), re.M))
        k = out[meta[".name"]]
        for short, key in KEYS:
            k[short] = int(meta[key])
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = sorted(set(old) | set(new))
    demangled = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    cols = [s for s, _ in KEYS] + ["loads", "waits"]
    print("kernel | " + " ".join(f"{c}(old>new)" for c in cols) + " | same")
    for name, pretty in zip(names, demangled):
        if name not in old or name not in new:
            print(f"{pretty.split('(')[0]} | only in {'old' if name in old else 'new'}")
            continue
        a, b = old[name], new[name]
        cells = " ".join(f"{a[c]}" if a[c] == b[c] else f"{a[c]}>{b[c]}" for c in cols)
        print(f"{pretty.split('(')[0].replace('void impop::', '')} | {cells} | {'same' if a['body'] == b['body'] else 'differs'}")


if __name__ == "__main__":
    main()
