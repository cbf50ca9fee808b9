"""Register, private-segment and LDS budget of every gfx950 kernel in a built libsplink_hip.so, read from the
code objects' metadata (no GPU needed); with two libraries, the kernels of the first whose budget grew in the second.

    python tools/kernel_resources.py [--brief] splink_amd/libsplink_hip.so [other/libsplink_hip.so]

--brief: rocprim's instantiations (a few thousand characters of template arguments each) are compared like the
rest but only counted in the output, unless one grew.

Each translation unit's code object is one entry of a clang offload bundle inside the library; the ELF note of
each holds .vgpr_count, .sgpr_count, .private_segment_fixed_size and .group_segment_fixed_size per kernel symbol.
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
READELF = os.environ.get("LLVM_READELF", "/opt/rocm/llvm/bin/llvm-readelf")


def code_objects(path):
    data = open(path, "rb").read()
    at = data.find(MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", data, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                yield data[at + off:at + off + size]
        at = data.find(MAGIC, at + len(MAGIC))


def resources(path):
    out = {}
    for obj in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(obj)
            f.flush()
            notes = subprocess.run([READELF, "--notes", f.name], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            name = re.search(r"\n\s+\.name:\s+(\S+)", block).group(1)
            out[name] = tuple(int(re.search(r"\n\s+%s:\s+(\d+)" % re.escape(f), block).group(1)) for f in FIELDS)
    return out


def main():
    brief = "--brief" in sys.argv
    paths = [x for x in sys.argv[1:] if x != "--brief"]
    a = resources(paths[0])
    b = resources(paths[1]) if len(paths) > 1 else None
    print(f"# {paths[0]}: {len(a)} kernels" + (f"; {paths[1]}: {len(b)} kernels" if b else ""))
    print("# kernel vgpr sgpr private_bytes lds_bytes" + (" | the same in the second library" if b else ""))
    grew, hidden = [], 0
    for name in sorted(a):
        if brief and "rocprim" in name and not (b and name in b and any(y > x for x, y in zip(a[name], b[name]))):
            hidden += 1
            continue
        line = f"{name} " + " ".join(map(str, a[name]))
        if b is not None:
            if name not in b:
                line += " | absent"
            else:
                line += " | " + " ".join(map(str, b[name]))
                if any(y > x for x, y in zip(a[name], b[name])):
                    grew.append(name)
                    line += "  GREW"
        print(line)
    if hidden:
        print(f"# and {hidden} rocprim instantiations" + (", none of which grew" if b is not None else ""))
    if b is not None:
        print(f"# new kernels: {sorted(set(b) - set(a))}")
        print(f"# kernels of the first library that grew in the second: {len(grew)} {grew}")
        return 1 if grew else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
