"""Instruction streams of two builds' kernels, matched by instantiation: which kernels are byte-identical, which differ,
which are new. Kernel names are demangled and a trailing template argument that one build added with its default
value is dropped before matching (`--drop-trailing-default "bool SC = false"` style: `--extra-arg false`), so that
decode_fused_kernel<..., 20> of the old build meets decode_fused_kernel<..., 20, false> of the new one. Instructions
are compared as text without addresses, and branch targets by offset within the kernel.

  python tools/isa_instantiation_diff.py OLD.o NEW.o [--extra-arg false]

OLD / NEW: host objects with a gfx950 offload bundle (slimt_amd/lib/obj/*.o) or gfx950 code objects.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"


def code_object(path, tmp):
    """the gfx950 code object of a host object's offload bundle (.hip_fatbin), else the file itself"""
    fb = os.path.join(tmp, os.path.basename(path) + ".fatbin")
    out = os.path.join(tmp, os.path.basename(path) + ".co")
    r = subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", path, os.path.join(tmp, "scratch.o")],
                       capture_output=True)
    if r.returncode != 0:
        return path
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}", f"--output={out}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True, capture_output=True)
    return out


def _trim(body):  # the padding behind a kernel's s_endpgm (up to the next kernel's alignment) is not its code
    while body and (body[-1].startswith(("s_nop", "s_code_end")) or body[-1] == "..."):
        body.pop()
    return body


def kernels(co):
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--demangle", co], capture_output=True,
                         text=True, check=True).stdout
    out, name, body = {}, None, []
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            if name:
                out[name] = _trim(body)
            name, body = m.group(1), []
            continue
        if name and line.strip() and not line.startswith("Disassembly"):
            ins = re.sub(r"//.*$", "", line).strip()
            ins = re.sub(r"<[^>]*>", "", ins)  # symbolic branch targets (label offsets stay)
            if ins and body and body[-1].startswith("s_getpc_b64") and ins.startswith("s_add_u32"):
                ins = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", ins)  # a call's distance: where the callee landed
            if ins:
                body.append(ins)
    if name:
        out[name] = _trim(body)
    return out


def key(name, extra):
    if extra:
        name = re.sub(r",\s*" + re.escape(extra) + r">\(", ">(", name)
    return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--extra-arg", default="")
    ap.add_argument("--match", default="")
    ap.add_argument("--pair", nargs=2, action="append", default=[], metavar=("OLD", "NEW"),
                    help="also compare the old kernel whose name contains OLD with the new one whose name contains NEW "
                         "(a kernel that became a template)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old = {key(k, ""): v for k, v in kernels(code_object(a.old, tmp)).items() if a.match in k}
        new_raw = {k: v for k, v in kernels(code_object(a.new, tmp)).items() if a.match in k}
    new = {key(k, a.extra_arg): v for k, v in new_raw.items()}
    same = [k for k in old if k in new and old[k] == new[k]]
    diff = [k for k in old if k in new and old[k] != new[k]]
    gone = [k for k in old if k not in new]
    added = [k for k in new_raw if key(k, a.extra_arg) not in old]
    for po, pn in a.pair:
        ko = next(k for k in old if po in k)
        kn = next(k for k in new_raw if pn in k)
        print("PAIR", "byte-identical" if old[ko] == new_raw[kn] else "DIFFERENT", ko, "->", kn)
        if old[ko] == new_raw[kn]:
            gone.remove(ko)
            added.remove(kn)
        else:
            diff.append(ko)
    print(f"{os.path.basename(a.old)}: {len(old)} kernels before, {len(new_raw)} after; "
          f"{len(same)} byte-identical, {len(diff)} different, {len(gone)} missing, {len(added)} new")
    for k in diff:
        print("DIFFERENT", k)
    for k in gone:
        print("MISSING", k)
    for k in sorted(added):
        print("NEW", k, f"({len(new_raw[k])} instructions)")
    return 1 if diff or gone else 0


if __name__ == "__main__":
    sys.exit(main())
