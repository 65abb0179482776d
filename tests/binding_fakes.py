"""What the *_cpu.py tests of the Python binding share, so that nothing a GPU would need is involved: include/bdpt.h as a C
compiler lays it out, a recording stand-in for libbdpt_amd.so, and what a GPU tensor looks like to the binding."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_layout(structs, consts=None, lang="c"):
    """include/bdpt.h as a C compiler reads it: {"<struct>": sizeof, "<struct>.<field>": offsetof, "<name>": the values of
    consts[name] (a list of C expressions) separated by spaces}, all as strings.  structs: {C name: field names}; lang: "c" (gcc) or "c++" (g++)
    compiles it."""
    lines = []
    for cname, fields in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f in fields]
    for name, exprs in (consts or {}).items():
        lines.append(f'printf("{name}{" %u" * len(exprs)}\\n", {", ".join(f"(unsigned)({e})" for e in exprs)});')
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "bdpt.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(c, "w").write(src)
        subprocess.run([{"c": "gcc", "c++": "g++"}[lang], "-x", lang, "-I", os.path.join(ROOT, "include"), "-o", exe, c],
                       check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return dict(re.findall(r"^(\S+) (.+)$", out, flags=re.M))


def desc_fields(d):
    """every field of a ctypes structure by name (an array as a list)"""
    return {n: (list(getattr(d, n)) if isinstance(getattr(d, n), C.Array) else getattr(d, n)) for n, _ in d._fields_}


class RecordingLib:
    """Stands in for libbdpt_amd.so behind a Context.  entry_points: {name: record}; a call of the entry point appends
    record(*arguments after the handle) to .calls and returns 0 (BDPT_OK).  A structure passed by reference arrives as the
    structure."""

    def __init__(self, entry_points, last_error=b""):
        self.calls, self._last_error = [], last_error
        for name, record in entry_points.items():
            setattr(self, name, self._entry_point(record))

    def _entry_point(self, record):
        def call(h, *args):
            self.calls.append(record(*[getattr(a, "_obj", a) for a in args]))
            return 0
        return call

    def bdpt_last_error(self, h):
        return self._last_error

    def bdpt_destroy(self, h):
        pass


def context_without_device(pkg, lib, device=0):
    ctx = pkg.Context.__new__(pkg.Context)
    ctx._lib, ctx._h, ctx.device = lib, C.c_void_p(1), device
    return ctx


class FakeGpuTensor:
    """What a GPU tensor looks like to the binding (no GPU needed)."""
    is_cuda = True

    def __init__(self, shape, dtype, index=0, contiguous=True, ptr=0x10000):
        import torch
        self.shape, self.dtype, self.device = tuple(shape), dtype, torch.device("cuda", index)
        self._contiguous, self._ptr = contiguous, ptr

    def is_contiguous(self):
        return self._contiguous

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(np.prod(self.shape))

    def data_ptr(self):
        return self._ptr

    def view(self, dtype):
        return self

    def __getitem__(self, k):
        return self


class _NullContext:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class _FakeOut(FakeGpuTensor):
    def __init__(self, shape, dtype):
        super().__init__(shape, dtype, ptr=0x90000)

    def cpu(self):
        return self

    def numpy(self):
        return np.zeros(self.shape, np.uint8)
