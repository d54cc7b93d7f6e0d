"""The host boundary of ``_C.so`` (CPU): every op's schema and dispatch keys are pinned against a
committed fixture, ``csrc/include/rn_api.h`` declares exactly the C-linkage launchers the library
defines, and no other prototype of one is left in the sources."""

import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from replicann_amd import _build

SO = Path(_build.OUT)
CSRC = Path(_build.CSRC)
API = CSRC / "include" / "rn_api.h"
FIXTURE = Path(__file__).resolve().parent / "fixtures" / "op_schemas.txt"
KEYS = ("CUDA", "CompositeExplicitAutograd")

pytestmark = pytest.mark.skipif(not SO.exists(), reason="extension not built")


def _registered():
    """``<schema> | <dispatch keys with a kernel>`` of every replicann::* op of the built library."""
    torch.ops.load_library(str(SO))
    lines = set()
    for name in torch._C._dispatch_get_all_op_names():
        if not name.startswith("replicann::"):
            continue
        base, _, overload = name.partition(".")
        keys = [k for k in KEYS if torch._C._dispatch_has_kernel_for_dispatch_key(name, k)]
        schemas = [s for s in torch._C._jit_get_schemas_for_operator(base) if s.overload_name == overload]
        assert len(schemas) == 1, name
        lines.add(f"{schemas[0]} | {','.join(keys)}")
    return lines


def test_op_schemas_and_dispatch_keys_are_pinned():
    """Names, schema strings and dispatch keys are the Python layer's contract with the library: a
    binding that moves between files must register exactly what it registered before."""
    want = set(FIXTURE.read_text().splitlines())
    got = _registered()
    assert len(want) == 78
    assert got == want, f"missing: {sorted(want - got)}\nunexpected: {sorted(got - want)}"
    assert sum(line.endswith("| CUDA") for line in got) == 56
    assert sum(line.endswith("| CompositeExplicitAutograd") for line in got) == 9


def _strip_comments(text):
    return re.sub(r"//[^\n]*", "", text)


def _declared():
    return set(re.findall(r"\b(rn_\w+)\s*\(", _strip_comments(API.read_text())))


@pytest.mark.skipif(shutil.which("nm") is None, reason="no nm")
def test_launcher_header_declares_what_the_library_defines():
    out = subprocess.run(["nm", "-D", "--defined-only", str(SO)], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in out.splitlines() if ln.split() and re.fullmatch(r"rn_\w+", ln.split()[-1])}
    declared = _declared()
    assert defined, "expected C-linkage launchers in the library"
    assert defined - declared == set(), f"defined but not declared in rn_api.h: {sorted(defined - declared)}"
    assert declared - defined == set(), f"declared in rn_api.h but not defined: {sorted(declared - defined)}"


def _sources():
    for d in ("kernels", "bindings", "comm", "include"):
        for p in sorted((CSRC / d).iterdir()):
            if p.suffix in (".hip", ".cpp", ".h"):
                yield p


def test_launchers_are_declared_in_one_place_only():
    declared = _declared()
    for p in _sources():
        text = p.read_text()
        if p == API:
            continue
        rel = p.relative_to(CSRC)
        if 'extern "C"' in text:
            assert '#include "rn_api.h"' in text, f'{rel} has extern "C" code but does not include rn_api.h'
        code = _strip_comments(text)
        used = set(re.findall(r"\b(rn_\w+)\s*\(", code)) & declared
        if used:
            assert '#include "rn_api.h"' in text, f"{rel} uses {sorted(used)[:3]} but does not include rn_api.h"
        for ln in code.splitlines():
            if 'extern "C"' in ln:
                assert not ln.rstrip().endswith(";"), f'{rel}: extern "C" prototype outside rn_api.h: {ln.strip()}'
        # a prototype inside an extern "C" block: an unindented `type rn_name(...);` of a declared launcher
        for m in re.finditer(r"^[A-Za-z_][^\n;{}()]*?\b(rn_\w+)\s*\([^;{}]*\)\s*;", code, re.M):
            assert m.group(1) not in declared, f"{rel}: prototype of {m.group(1)} outside rn_api.h"
