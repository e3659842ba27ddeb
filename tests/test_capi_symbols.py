"""The C-ABI shared library loads on a GPU-less host and exports exactly what include/fokl_hip.h (the boundary) and
include/fokl_hip_internal.h (this package's own plumbing) declare."""
import ctypes
import os
import re

import pytest

from helpers import ROOT
from fokl_gpy_amd import _capi

HEADER = os.path.join(ROOT, 'include', 'fokl_hip.h')                       # the C ABI: what a maintainer binds
INTERNAL = os.path.join(ROOT, 'include', 'fokl_hip_internal.h')            # this package's own plumbing (_capi.py only)


def declared_symbols(path=HEADER):
    text = open(path).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(fokl_[a-z0-9_]+)\s*\(', text)))


def test_header_declares_the_documented_entry_points():
    syms = declared_symbols()
    for must in ('fokl_ctx_create', 'fokl_upload', 'fokl_build_terms', 'fokl_gram', 'fokl_bic_resid',
                 'fokl_gibbs_chain', 'fokl_predict', 'fokl_comm_allgather_f64', 'fokl_comm_allreduce_sum_f64'):
        assert must in syms


def test_the_boundary_is_separate_from_the_plumbing():
    """include/fokl_hip.h is the stable boundary (SURVEY 8(b)'s set + the K1-K3 launch forms, predict, derivatives, clean,
    GP_Integrate, comm); the search / pool / stream / device-engine plumbing lives in fokl_hip_internal.h and nowhere else."""
    public, internal = declared_symbols(HEADER), declared_symbols(INTERNAL)
    assert not set(public) & set(internal)
    prefixes = ('fokl_search_', 'fokl_pool_', 'fokl_stream_', 'fokl_dchain_', 'fokl_dspectral_', 'fokl_outcome_',
                'fokl_spectrum_')
    assert not [s for s in public if s.startswith(prefixes)]
    assert len(public) <= 50
    # both headers are plain C (the boundary needs nothing of the plumbing)
    import shutil
    import subprocess
    cc = shutil.which('gcc') or shutil.which('cc')
    if cc:
        for header in (HEADER, INTERNAL):
            res = subprocess.run([cc, '-fsyntax-only', '-x', 'c', '-std=c99', '-Wall', header], capture_output=True, text=True)
            assert res.returncode == 0, res.stderr


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(_capi.LIB_PATH)
    missing = [s for s in declared_symbols(HEADER) + declared_symbols(INTERNAL) if not hasattr(lib, s)]
    assert missing == []


def test_binding_table_matches_header():
    assert sorted(_capi.SIGNATURES.keys()) == sorted(declared_symbols(HEADER) + declared_symbols(INTERNAL))


def declared_functions(path):
    """{name: [parameter text, ...]} of every function a header declares ((void): no parameter)."""
    text = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r'\b(fokl_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;', text):
        params = ' '.join(params.split())
        out[name] = [] if params in ('', 'void') else [part.strip() for part in params.split(',')]
    return out


def parameter_class(text):
    """'pointer', 'double', 'int64' or 'int32' of a C parameter as the headers write them."""
    if '*' in text or '[' in text:
        return 'pointer'
    kind = text.split()[-2] if len(text.split()) > 1 else text
    return {'double': 'double', 'int64_t': 'int64', 'uint64_t': 'int64', 'size_t': 'int64', 'int': 'int32', 'int32_t': 'int32',
            'uint32_t': 'int32', 'unsigned': 'int32'}[kind]


def ctypes_class(kind):
    if kind in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(kind, ctypes._Pointer):
        return 'pointer'
    if kind is ctypes.c_double:
        return 'double'
    assert issubclass(kind, ctypes._SimpleCData) and kind._type_ in 'iIlLqQ', kind
    return 'int64' if ctypes.sizeof(kind) == 8 else 'int32'


SYSTEM_CALLS = ('fokl_simulate_ensemble', 'fokl_simulate_adaptive', 'fokl_simulate_stiff', 'fokl_assimilate_ensemble',
                'fokl_control_solve', 'fokl_control_pooled_solve', 'fokl_control_cvar_solve')
SYSTEM_REPORTS = ('fokl_simulate_report', 'fokl_simulate_adaptive_report', 'fokl_simulate_stiff_report', 'fokl_assimilate_report',
                  'fokl_control_report', 'fokl_control_pooled_report', 'fokl_control_cvar_report')


def test_binding_signatures_match_the_headers():
    """Every declared function without a function-pointer parameter has as many argtypes as parameters; for the calls that
    take a fokl_system and their reports every parameter's class (pointer, double, 64-bit, 32-bit integer) matches too."""
    declared = {**declared_functions(HEADER), **declared_functions(INTERNAL)}
    assert sorted(declared) == sorted(_capi.SIGNATURES)
    miscounted = {name: (len(params), len(_capi.SIGNATURES[name][1])) for name, params in declared.items()
                  if not any('(' in p for p in params) and len(params) != len(_capi.SIGNATURES[name][1])}
    assert miscounted == {}
    for name in SYSTEM_CALLS + SYSTEM_REPORTS:
        header = [parameter_class(p) for p in declared[name]]
        binding = [ctypes_class(kind) for kind in _capi.SIGNATURES[name][1]]
        assert header == binding, name


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof and every offsetof of fokl_system and fokl_control_problem as a C compiler lays them out equal the ctypes
    classes', field by field and by name."""
    import shutil
    import subprocess
    cc = shutil.which('gcc') or shutil.which('cc')
    assert cc, "no C compiler: the layout of the structs cannot be checked"
    structs = {'fokl_system': _capi._SystemStruct, 'fokl_control_problem': _capi._ControlProblemStruct}
    lines = []
    for c_name, cls in structs.items():
        lines.append(f'    printf("{c_name} sizeof %zu\\n", sizeof({c_name}));')
        lines += [f'    printf("{c_name} {field} %zu\\n", offsetof({c_name}, {field}));' for field, _ in cls._fields_]
    source = tmp_path / 'layout.c'
    source.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "fokl_hip_internal.h"\nint main(void)\n{\n' +
                      '\n'.join(lines) + '\n    return 0;\n}\n')
    program = tmp_path / 'layout'
    res = subprocess.run([cc, '-std=c99', '-Wall', '-I', os.path.dirname(INTERNAL), '-o', str(program), str(source)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    printed = subprocess.run([str(program)], capture_output=True, text=True, check=True).stdout.split('\n')
    in_c = {(s, f): int(v) for s, f, v in (line.split() for line in printed if line)}
    in_python = {}
    for c_name, cls in structs.items():
        in_python[(c_name, 'sizeof')] = ctypes.sizeof(cls)
        in_python.update({(c_name, field): getattr(cls, field).offset for field, _ in cls._fields_})
    assert in_python == in_c
    # and the classes name every field the header has: a field missing in Python would shift nothing it checks above
    text = re.sub(r'/\*.*?\*/', '', open(INTERNAL).read(), flags=re.S)
    for c_name, cls in structs.items():
        body = re.search(r'typedef struct ' + c_name + r' \{(.*?)\} ' + c_name + ';', text, flags=re.S).group(1)
        fields = [name for decl in body.split(';') for name in re.findall(r'(\w+)\s*(?:,|$)', decl.strip())]
        assert fields == [field for field, _ in cls._fields_], c_name


def test_no_device_is_reported_not_hidden():
    """Without a GPU the context constructor must raise (no CPU fallback); with one it must succeed."""
    n = _capi.device_count()
    if n == 0:
        try:
            _capi.DeviceContext(0)
        except _capi.FoklNativeError as exc:
            assert exc.code == -1
        else:
            raise AssertionError("DeviceContext(0) succeeded without a device")
    else:
        ctx = _capi.DeviceContext(0)
        ctx.close()


def test_version():
    assert _capi.load().fokl_version() >= 100


def test_development_build_of_the_hip_translation_unit_still_parses():
    """`make DEV=1` (the retired Gram kernels kept for A/B runs, -DFOKL_DEV_KERNELS) shares fokl_hip.hip with the product
    build: a host-side syntax pass over it catches an edit that only compiles without the flag."""
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    src = os.path.join(os.path.dirname(os.path.abspath(_capi.__file__)), 'csrc', 'fokl_hip.hip')
    res = subprocess.run([hipcc, '-std=c++17', '-ffp-contract=off', '--offload-arch=gfx950', '-DFOKL_DEV_KERNELS',
                          '--cuda-host-only', '-fsyntax-only', '-Wno-unused-command-line-argument', src],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
