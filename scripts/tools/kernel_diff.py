"""Device code of two builds of the library, kernel by kernel: is it the same?

  python scripts/tools/kernel_diff.py <_obj dir A> <_obj dir B>

Every object of both directories is unbundled to its gfx950 code object (as kernel_regs.py does); the kernels of the whole library are keyed on
their mangled names -- a kernel may move between objects -- and compared on
  * the set of names,
  * the metadata of each: VGPR, AGPR, SGPR, spill count, scratch, LDS, kernarg size,
  * the raw bytes of the kernel's symbol and of its descriptor (<name>.kd).  One field of the descriptor is an address: kernel_code_entry_byte_offset
    (bytes 16 .. 23), the distance from the descriptor to the code, which changes when kernels are laid out in another order; it is left out of the
    comparison and the kernels where it differs are counted.
Relocations in a code object would make a byte comparison meaningless: they are counted and reported.  Exit status 0 = identical.
"""
import os
import re
import subprocess
import sys
import tempfile

from kernel_regs import LLVM, unbundle

META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size",
        "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size")


def readelf(*args):
    return subprocess.run([LLVM + "/llvm-readelf", "--wide"] + list(args), capture_output=True, text=True, check=True).stdout


def code_object(obj):
    """{kernel name: (metadata dict, code bytes, descriptor bytes)}, relocation count of one object file's gfx950 code object"""
    with tempfile.TemporaryDirectory() as d:
        co = os.path.join(d, "a.co")
        if not unbundle(obj, co):
            return {}, 0
        notes, syms, secs, rel = readelf("--notes", co), readelf("--symbols", co), readelf("--section-headers", co), readelf("--relocations", co)
        with open(co, "rb") as f:
            image = f.read()
    sections = {}       # index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+(\S+)\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", secs, re.M):
        if m.group(2) != "NOBITS":
            sections[int(m.group(1))] = (int(m.group(3), 16), int(m.group(4), 16))
    extent = {}         # symbol -> bytes
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)$", syms, re.M):
        addr, size, ndx, name = int(m.group(1), 16), int(m.group(2)), int(m.group(4)), m.group(5)
        if ndx in sections:
            off = addr - sections[ndx][0] + sections[ndx][1]
            extent[name] = image[off:off + size]
    out = {}
    for k in re.split(r"\n(?=\s+- \.agpr_count)", notes)[1:]:
        g = lambda key: re.search(r"\.%s:\s+(\S+)" % key, k)      # noqa: E731
        name = g("name").group(1)
        out[name] = ({key: g(key).group(1) for key in META if g(key)}, extent[name], extent[name + ".kd"])
    return out, len(re.findall(r"^[0-9a-f]{8,16}\s+[0-9a-f]{8,16}\s+R_", rel, re.M))


def library(obj_dir):
    kernels, where, relocs = {}, {}, 0
    for f in sorted(os.listdir(obj_dir)):
        if not f.endswith(".o") or f == "source_hash.o":
            continue
        ks, r = code_object(os.path.join(obj_dir, f))
        relocs += r
        for name, k in ks.items():
            assert name not in kernels, "kernel %s in both %s and %s" % (name, where[name], f)
            kernels[name], where[name] = k, f
    return kernels, where, relocs


if __name__ == "__main__":
    (a, where_a, rel_a), (b, where_b, rel_b) = library(sys.argv[1]), library(sys.argv[2])
    bad = 0
    for name in sorted(set(a) ^ set(b)):
        bad += 1
        print("only in %s: %s (%s)" % ("A" if name in a else "B", name, (where_a if name in a else where_b)[name]))
    moved = placed = 0
    for name in sorted(set(a) & set(b)):
        (ma, ca, da), (mb, cb, db) = a[name], b[name]
        moved += where_a[name] != where_b[name]
        if ma != mb:
            bad += 1
            print("metadata differs: %s\n  A %s\n  B %s" % (name, ma, mb))
        if ca != cb:
            bad += 1
            n = sum(x != y for x, y in zip(ca, cb))
            print("code differs: %s (%d / %d bytes; %d differing)" % (name, len(ca), len(cb), n))
        if da[:16] + da[24:] != db[:16] + db[24:]:
            bad += 1
            print("descriptor differs: %s" % name)
        placed += da[16:24] != db[16:24]
    print("kernels: A %d, B %d, common %d (in another object: %d); code bytes compared: %d; relocations: A %d, B %d; "
          "descriptors with another entry offset: %d; differences: %d"
          % (len(a), len(b), len(set(a) & set(b)), moved, sum(len(a[n][1]) for n in set(a) & set(b)), rel_a, rel_b, placed, bad))
    sys.exit(1 if bad else 0)
