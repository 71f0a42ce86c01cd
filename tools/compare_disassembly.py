#!/usr/bin/env python3
"""Are the gfx950 kernels two builds of the library share identical, instruction for instruction?

    python tools/compare_disassembly.py OLD.so NEW.so

Every code object of both libraries' .hip_fatbin sections is unbundled and disassembled (llvm-objdump -d); per kernel symbol the
instruction text (addresses and encodings dropped, so a kernel may move inside its code object) is compared.  Prints the kernels only
one side has and the kernels whose text differs; exit status 1 if a kernel both sides have differs or one of OLD's is gone."""
import collections
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def kernels(lib):
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
                name = None
                for line in text.splitlines():
                    m = re.match(r"^[0-9a-f]* ?<(\S+)>:$", line.strip())
                    if m:
                        name = m.group(1)
                        out.setdefault(name, [])
                    elif name and line.strip():
                        out[name].append(re.sub(r"\s*//.*$", "", line).strip())      # drop the address comments
    return out


if __name__ == "__main__":
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    gone = [k for k in old if k not in new]
    added = [k for k in new if k not in old]
    differ = [k for k in old if k in new and old[k] != new[k]]
    print(f"{len(old)} symbols in {sys.argv[1]}, {len(new)} in {sys.argv[2]}: {len(old) - len(gone) - len(differ)} identical, "
          f"{len(differ)} differ, {len(gone)} gone, {len(added)} added")
    for title, names in (("differ", differ), ("gone", gone), ("added", added)):
        for k in names:
            print(f"  {title}: {subprocess.run(['c++filt', k], capture_output=True, text=True).stdout.strip()[:150]}")
    sys.exit(1 if differ or gone else 0)
