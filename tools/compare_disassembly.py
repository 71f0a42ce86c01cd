#!/usr/bin/env python3
"""Are the gfx950 kernels two builds of the library share identical, instruction for instruction?

    python tools/compare_disassembly.py OLD.so NEW.so
    python tools/compare_disassembly.py --registers [--only REGEX] OLD.so NEW.so

Every code object of both libraries' .hip_fatbin sections is unbundled and disassembled (llvm-objdump -d); per kernel symbol the
instruction text (addresses and encodings dropped, so a kernel may move inside its code object) is compared.  Prints the kernels only
one side has and the kernels whose text differs; exit status 1 if a kernel both sides have differs or one of OLD's is gone.

--registers also compares the text with register numbers replaced by placeholders (v12 -> v, s[4:5] -> s[]) and prints, for every kernel
whose demangled name matches --only (default: all), its class -- identical, identical up to register names, different -- and the
resources both builds' code-object notes state for it (VGPRs, SGPRs, LDS bytes, scratch bytes).  Exit status 1 if a kernel is different,
one of OLD's is gone, or a kernel that is identical only up to register names needs more of any resource than OLD's."""
import collections
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


RESOURCES = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("lds", ".group_segment_fixed_size"), ("scratch", ".private_segment_fixed_size"))


def notes(co, meta):
    """The resources of every kernel of one code object, from its notes (amdhsa.kernels, printed as YAML)."""
    text = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    entry, top = None, None
    for line in text.splitlines():
        m = re.match(r"^(\s*)(- )?(\.\w+):\s*(\S*)", line)
        if not m:
            continue
        indent = len(m.group(1))
        if m.group(2) and (top is None or indent <= top) and m.group(3) == ".agpr_count":    # keys are sorted: a kernel's entry starts here
            top, entry = indent, {}
        if entry is not None and indent == top + (0 if m.group(2) else 2):
            entry[m.group(3)] = m.group(4)
            if m.group(3) == ".symbol":
                meta[m.group(4).strip("'\"")[:-len(".kd")]] = entry
    return meta


def normalised(lines):
    return [re.sub(r"\b([vsa])\[\d+:\d+\]", r"\1[]", re.sub(r"\b([vsa])\d+\b", r"\1", l)) for l in lines]


def kernels(lib, meta=None):
    out = collections.OrderedDict()
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fatbin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for i, s in enumerate(starts):
            one = os.path.join(d, f"bundle{i}")
            open(one, "wb").write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            targets = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--list", "--type=o", f"--input={one}"],
                                     check=True, capture_output=True, text=True).stdout.split()
            for t in targets:
                if "gfx" not in t:
                    continue
                co = one + ".co"
                subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={t}",
                                       f"--input={one}", f"--output={co}"])
                text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                                      check=True, capture_output=True, text=True).stdout
                if meta is not None:
                    notes(co, meta)
                name = None
                for line in text.splitlines():
                    m = re.match(r"^[0-9a-f]* ?<(\S+)>:$", line.strip())
                    if m:
                        name = m.group(1)
                        out.setdefault(name, [])
                    elif name and line.strip():
                        out[name].append(re.sub(r"\s*//.*$", "", line).strip())      # drop the address comments
    return out


def demangled(k):
    return subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip()


def by_registers(args):
    only = re.compile(args[args.index("--only") + 1]) if "--only" in args else None
    libs = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--only")]
    old_meta, new_meta = {}, {}
    old, new = kernels(libs[0], old_meta), kernels(libs[1], new_meta)
    bad = False
    counts = collections.Counter()
    print(f"{'kernel':58s} {'class':34s} " + " ".join(f"{n + ' old>new':>16s}" for n, _ in RESOURCES))
    for k in old:
        name = demangled(k)
        if k not in old_meta or (only and not only.search(name)):
            continue
        if k not in new:
            print(f"{name[:58]:58s} gone")
            bad = True
            continue
        cls = ("identical" if old[k] == new[k] else
               "identical up to register names" if normalised(old[k]) == normalised(new[k]) else "different")
        res = [(int(old_meta[k][key]), int(new_meta[k][key])) for _, key in RESOURCES]
        more = any(b > a for a, b in res)
        bad |= cls == "different" or (cls != "identical" and more)
        counts[cls] += 1
        print(f"{name[:58]:58s} {cls:34s} " + " ".join(f"{f'{a}>{b}':>16s}" for a, b in res) + ("   MORE" if more else ""))
    print(", ".join(f"{n} {c}" for c, n in counts.items()))
    return 1 if bad else 0


if __name__ == "__main__":
    if "--registers" in sys.argv:
        sys.exit(by_registers(sys.argv[1:]))
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    gone = [k for k in old if k not in new]
    added = [k for k in new if k not in old]
    differ = [k for k in old if k in new and old[k] != new[k]]
    print(f"{len(old)} symbols in {sys.argv[1]}, {len(new)} in {sys.argv[2]}: {len(old) - len(gone) - len(differ)} identical, "
          f"{len(differ)} differ, {len(gone)} gone, {len(added)} added")
    for title, names in (("differ", differ), ("gone", gone), ("added", added)):
        for k in names:
            print(f"  {title}: {demangled(k)[:150]}")
    sys.exit(1 if differ or gone else 0)
