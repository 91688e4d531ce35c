#!/usr/bin/env python3
"""The gfx950 kernels of an object file or a library, read with the ROCm LLVM tools.

  python tools/kernel_shape.py gemm 'gemm2_kernelIDF16bLi1[29][82]ELi128ELi4'
      size, branch count, registers and scratch of the kernels of csrc/obj/<unit>.o whose mangled name matches the pattern
  python tools/kernel_shape.py --compare [--accept-shape] OLD NEW
      two object files or libraries, per kernel symbol: are the instruction bytes equal, is the metadata equal (vgpr / sgpr /
      agpr counts, group and private segment sizes, kernarg size, max flat workgroup size), and is the SHAPE equal: LDS, scratch,
      kernarg and workgroup sizes, the waves per SIMD the register count permits, and the counts of MFMA, LDS-DMA, LDS read,
      LDS write, workgroup-barrier, global-load and global-store instructions.  Symbols on one side only are listed.
      Exit status 0 only when both sides hold the same symbols with equal bytes and equal metadata; with --accept-shape a
      kernel whose shape is equal passes too (a refactor that moved the compiler's schedule but not the kernel's resources).
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "kernarg_segment_size", "max_flat_workgroup_size")
SHAPE_META = ("group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size")
# instruction classes of the shape verdict, by mnemonic prefix; the first class that matches takes the instruction
CLASSES = (("mfma", ("v_mfma",)), ("lds_dma", ("global_load_lds",)), ("lds_read", ("ds_read",)),
           ("lds_write", ("ds_write",)), ("barrier", ("s_barrier",)), ("global_load", ("global_load", "flat_load")),
           ("global_store", ("global_store", "flat_store")))


def _out(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout


def code_objects(path, tmp):
    """The gfx950 code objects of `path` (one offload bundle per translation unit in its .hip_fatbin section), as files."""
    tag = hashlib.sha1(os.path.abspath(path).encode()).hexdigest()[:8]
    fat = os.path.join(tmp, tag + ".fat")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", path, os.path.join(tmp, tag + ".copy")], check=True)
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", blob)]
    cos = []
    for k, a in enumerate(starts):
        piece, co = os.path.join(tmp, f"{tag}.{k}.bin"), os.path.join(tmp, f"{tag}.{k}.co")
        open(piece, "wb").write(blob[a:starts[k + 1] if k + 1 < len(starts) else len(blob)])
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={piece}", f"--output={co}"], check=True)
        cos.append(co)
    return cos


def metadata(co):
    """{kernel name: {key: value}} from the code object's AMDGPU metadata note."""
    kernels, cur = {}, None
    for line in _out(f"{LLVM}/llvm-readelf", "--notes", co).splitlines():
        if re.match(r"  - \.", line):          # a new entry of amdhsa.kernels
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"    \.(\w+):\s*(\S+)$", line)
        if cur is not None and m:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                kernels[m.group(2)] = cur
    return kernels


def kernel_bytes(co):
    """{kernel name: its instruction bytes}: the FUNC symbols of the code object, cut out of their section."""
    data = open(co, "rb").read()
    sections = {}
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s", _out(f"{LLVM}/llvm-readelf", "-S", "--wide", co), re.M):
        sections[m.group(1)] = (int(m.group(2), 16), int(m.group(3), 16))
    out = {}
    for line in _out(f"{LLVM}/llvm-readelf", "-s", "--wide", co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6] in sections:
            addr, off = sections[f[6]]
            start = int(f[1], 16) - addr + off
            out[f[7]] = data[start:start + int(f[2])]
    return out


def waves_per_simd(meta):
    """Waves per SIMD the register allocation permits: 512 registers in blocks of 8, at most 8 waves."""
    return min(8, 512 // max(8, -(-int(meta["vgpr_count"]) // 8) * 8)) if "vgpr_count" in meta else None


def class_counts(co):
    """{kernel name: {instruction class: count}} from the code object's disassembly."""
    lines = _out(f"{LLVM}/llvm-objdump", "-d", co).split("\n")
    starts = [i for i, l in enumerate(lines) if re.match(r"^[0-9a-f]+ <\S+>:$", l)] + [len(lines)]
    out = {}
    for i, j in zip(starts, starts[1:]):
        counts = dict.fromkeys((c for c, _ in CLASSES), 0)
        for l in lines[i + 1:j]:
            mnemonic = l.split()[0] if l.split() else ""
            for c, prefixes in CLASSES:
                if mnemonic.startswith(prefixes):
                    counts[c] += 1
                    break
        out[lines[i].split("<")[1].rstrip(">:")] = counts
    return out


def compare(old, new, accept_shape=False):
    with tempfile.TemporaryDirectory() as tmp:
        sides = []
        for path in (old, new):
            code, meta, counts = {}, {}, {}
            for k, co in enumerate(code_objects(path, tmp)):
                m, n = metadata(co), class_counts(co)
                for name, b in kernel_bytes(co).items():
                    key = name if name not in code else f"{name} [code object {k}]"     # a static kernel of several units
                    code[key], meta[key], counts[key] = b, m.get(name, {}), n.get(name, {})
            sides.append((code, meta, counts))
    (c0, m0, n0), (c1, m1, n1) = sides
    both = sorted(set(c0) & set(c1))
    bad = n_bytes = n_shape = 0
    for name in both:
        same_code = c0[name] == c1[name]
        k0, k1 = ({k: m[name].get(k) for k in META} for m in (m0, m1))
        s0, s1 = ({**{k: m[name].get(k) for k in SHAPE_META}, "waves_per_simd": waves_per_simd(m[name]), **n[name]}
                  for m, n in ((m0, n0), (m1, n1)))
        n_bytes += same_code
        n_shape += s0 == s1
        bad += not ((same_code and k0 == k1) or (accept_shape and s0 == s1))
        diff = ", ".join(f"{k} {k0[k]} -> {k1[k]}" for k in META if k0[k] != k1[k])
        sdiff = ", ".join(f"{k} {s0[k]} -> {s1[k]}" for k in s0 if s0[k] != s1.get(k))
        print(f"{name}  bytes {'equal' if same_code else 'DIFFERENT'} ({len(c0[name])} / {len(c1[name])}, sha256 "
              f"{hashlib.sha256(c1[name]).hexdigest()[:12]})  metadata {'equal' if k0 == k1 else 'DIFFERENT: ' + diff}"
              f"  shape {'equal' if s0 == s1 else 'DIFFERENT: ' + sdiff}")
    only = [(n, "first") for n in sorted(set(c0) - set(c1))] + [(n, "second") for n in sorted(set(c1) - set(c0))]
    for name, side in only:
        print(f"{name}  only in the {side}")
    print(f"{len(both)} symbols on both sides, {n_bytes} with equal bytes, {n_shape} with equal shape "
          f"({n_shape - n_bytes} shape only), {bad} fail, {len(only)} on one side only")
    return 0 if both and not bad and not only else 1


def shape(unit, pattern):
    pat = re.compile(pattern)
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(os.path.join(ROOT, "ubisoft-laforge-msmd_amd", "csrc", "obj", unit + ".o"), tmp):
            meta = metadata(co)
            lines = _out(f"{LLVM}/llvm-objdump", "-d", co).split("\n")
            starts = [i for i, l in enumerate(lines) if re.match(r"^[0-9a-f]+ <_Z", l)] + [len(lines)]
            for i, j in zip(starts, starts[1:]):
                name = lines[i].split("<")[1].rstrip(">:")
                if pat.search(name):
                    r = meta.get(name, {})
                    branches = sum("s_cbranch" in b or "s_branch" in b for b in lines[i:j])
                    print(f"{name[:100]:100s} lines {j - i:6d} branches {branches:5d} vgpr {r.get('vgpr_count')} "
                          f"scratch {r.get('private_segment_fixed_size')}")


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--compare":
        paths = [a for a in sys.argv[2:] if a != "--accept-shape"]
        sys.exit(compare(paths[0], paths[1], accept_shape="--accept-shape" in sys.argv[2:]))
    shape(sys.argv[1] if len(sys.argv) > 1 else "gemm", sys.argv[2] if len(sys.argv) > 2 else "gemm2_kernel")
