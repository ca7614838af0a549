#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libacfm_hip.so, kernel by kernel.

    tools/isa_diff.py OLD NEW [--diag] [--allow-removed NAME ...] [--show N]

OLD / NEW: a library, or a source tree (then <tree>/acfm_video_3d_reconstruction_amd/libacfm_hip.so, with
--diag libacfm_hip_diag.so; build it first with the csrc Makefile).  Kernels are matched by mangled name over all
code objects of a library, so moving a kernel between translation units is not a difference.  Two kernels are
identical when their instruction sequences agree (disassembly without addresses and encodings, local labels
renumbered in order of appearance, trailing padding dropped) and their descriptors agree (VGPRs, AGPRs, SGPRs,
LDS bytes, scratch bytes, wavefront size, kernarg bytes).  Exit status 0: every kernel of OLD is in NEW and
identical, except the ones named with --allow-removed (substring of the mangled name), and NEW adds none.
Needs only the ROCm prefix's llvm-objdump and llvm-readelf ($ROCM_PATH, default /opt/rocm).
"""
import argparse
import difflib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
DESC_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
             "wavefront_size", "kernarg_segment_size")
PADDING = ("s_code_end", "s_nop 0", "...")   # what the assembler puts behind a kernel's last s_endpgm


def code_objects(lib):
    """The gfx950 ELF images of every offload bundle in the library (one bundle per translation unit)."""
    blob = open(lib, "rb").read()
    out, i = [], blob.find(MAGIC)
    while i >= 0:
        (count,) = struct.unpack_from("<Q", blob, i + len(MAGIC))
        p = i + len(MAGIC) + 8
        for _ in range(count):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                out.append(blob[i + off:i + off + size])
        i = blob.find(MAGIC, i + len(MAGIC))
    return out


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def kernels_of(lib):
    """{mangled name: (normalised instruction list, descriptor dict)}"""
    result = {}
    with tempfile.TemporaryDirectory() as tmp:
        for n, image in enumerate(code_objects(lib)):
            path = os.path.join(tmp, "co%d.elf" % n)
            open(path, "wb").write(image)
            desc, cur = {}, None
            for line in run("llvm-readelf", "--notes", path).splitlines():
                if re.match(r"^  - \.", line):
                    cur = {}
                m = re.match(r"^(?:  - |    )\.(\w+):\s+(\S+)$", line)   # kernel-level keys only (arguments sit deeper)
                if m and cur is not None:
                    cur[m.group(1)] = m.group(2)
                    if m.group(1) == "symbol":
                        desc[m.group(2)[:-3] if m.group(2).endswith(".kd") else m.group(2)] = cur
            text, sym = {}, None
            for line in run("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", "--symbolize-operands",
                            path).splitlines():
                m = re.match(r"^<(\w+)>:$", line)
                if m and not re.fullmatch(r"L\d+", m.group(1)):
                    sym = m.group(1)
                    text[sym] = []
                elif sym is not None and line.strip():
                    text[sym].append(re.sub(r"\s*//.*$", "", line).strip())
            for sym, d in desc.items():
                ins = text.get(sym, [])
                while ins and ins[-1] in PADDING:
                    ins.pop()
                labels = {}
                for s in ins:
                    for lab in re.findall(r"\bL\d+\b", s):
                        labels.setdefault(lab, "L%d" % len(labels))
                ins = [re.sub(r"\bL\d+\b", lambda m: labels[m.group(0)], s) for s in ins]
                assert sym not in result, "kernel %s is emitted by two code objects of %s" % (sym, lib)
                result[sym] = (ins, {k: d.get(k) for k in DESC_KEYS})
    return result


def resolve(path, diag):
    if os.path.isdir(path):
        path = os.path.join(path, "acfm_video_3d_reconstruction_amd", "libacfm_hip_diag.so" if diag else "libacfm_hip.so")
    if not os.path.isfile(path):
        sys.exit("isa_diff: no library at %s (build it first)" % path)
    return path


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--diag", action="store_true", help="for trees: compare the DIAG=1 libraries")
    ap.add_argument("--allow-removed", nargs="*", default=[], metavar="NAME")
    ap.add_argument("--show", type=int, default=40, help="diff lines printed per differing kernel")
    a = ap.parse_args()
    old, new = kernels_of(resolve(a.old, a.diag)), kernels_of(resolve(a.new, a.diag))
    names = sorted(set(old) | set(new))
    pretty = {k: k for k in names}   # mangled: the ROCm prefix ships no demangler, and the names read well enough
    same, bad, removed = 0, 0, 0
    for k in names:
        if k not in new:
            ok = any(x in k for x in a.allow_removed)
            removed += ok
            bad += not ok
            print("%s  %s" % ("removed  " if ok else "MISSING  ", pretty[k]))
        elif k not in old:
            bad += 1
            print("ADDED     %s" % pretty[k])
        elif old[k] == new[k]:
            same += 1
        else:
            bad += 1
            print("DIFFERS   %s" % pretty[k])
            for key in DESC_KEYS:
                if old[k][1][key] != new[k][1][key]:
                    print("    %s: %s -> %s" % (key, old[k][1][key], new[k][1][key]))
            for line in list(difflib.unified_diff(old[k][0], new[k][0], "old", "new", n=2, lineterm=""))[:a.show]:
                print("    " + line)
    print("%d kernels identical, %d removed%s" % (same, removed, ", %d DIFFERENT / missing / added" % bad if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
