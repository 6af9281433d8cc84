"""One-off (README.md): the gfx950 kernels inside two libexmc_hip.so builds, compared per kernel symbol --
names, instruction text, and the register / scratch / LDS figures of the kernels' metadata.
    python profiles/host_split/compare_device_code.py PARENT.so RESULT.so    (llvm-objdump, llvm-readelf on PATH)"""
import re
import shutil
import subprocess
import sys
import tempfile

FIGURES = ("agpr_count", "vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count",
           "private_segment_fixed_size", "group_segment_fixed_size", "kernarg_segment_size")


def run(d, *cmd):
    return subprocess.run(cmd, cwd=d, capture_output=True, text=True, check=True).stdout


def kernels(so):
    """{kernel: (figures, [instruction, ...])} over every gfx950 code object in `so`"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(so, d + "/lib.so")
        run(d, "llvm-objdump", "--offloading", "lib.so")
        for co in run(d, "ls").split():
            if "gfx950" not in co:
                continue
            text, fn = {}, None
            for ln in run(d, "llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
                m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", ln)
                ln = re.sub(r"<L\d+>", "<L>", re.sub(r"\s*//.*$", "", ln).strip())
                if m and not re.match(r"L\d+$", m.group(1)):
                    fn = m.group(1)
                    text[fn] = []
                elif fn and ln:
                    # not code: how far a table or function lies from this instruction inside the code object
                    if text[fn] and text[fn][-1].startswith("s_getpc_b64") and re.match(r"s_add_u32 (\S+), \1, 0x", ln):
                        ln = re.sub(r"0x[0-9a-f]+$", "<pcrel>", ln)
                    text[fn].append("<L>:" if m else ln)
            for t in text.values():                # nor is the padding after a code object's last function
                while t and t[-1] == "s_nop 0":
                    t.pop()
            for blk in run(d, "llvm-readelf", "--notes", co).split("  - .agpr_count:")[1:]:
                f = dict(re.findall(r"\.(\w+):\s+(\S+)", ".agpr_count:" + blk))
                out[f["name"]] = (tuple(f.get(k) for k in FIGURES), text[f["name"]])
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
print("kernels:", len(a), "->", len(b), "; names only in one:", sorted(set(a) ^ set(b)))
differ = [k for k in sorted(set(a) & set(b)) if a[k] != b[k]]
print("instructions compared:", sum(len(v[1]) for v in a.values()))
print("identical:", len(set(a) & set(b)) - len(differ), "different:", differ)
