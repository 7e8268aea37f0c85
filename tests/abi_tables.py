"""The harness of the two kinds of ABI-table tests, which every C entry point of the trunk gets: what it REFUSES
(``test_capi_refusals*.py``) and what its launcher HANDS OVER (``test_launch_marshalling*.py``).  A test file keeps what is its own --
its ``table()`` or ``cases()``, the child entry under ``__main__``, the tests of its particular rows -- and hands the table to this
module, which runs it, checks what the table promises of its own rows, and compares the result with the file's golden JSON
(``golden/make_golden_abi.py`` writes those, through the same functions).

Refusals.  Per entry point one valid base call with fake pointers (``Entry``) and rows that each change one argument, or two where the
point is the ORDER of the checks.  NO row may reach a kernel launch: the pointers address nothing.  The table runs in ONE fresh child
process that sees no GPU and says so (``opa_device_count() == 0``) before its first row: a check that a later change drops meets "no
device" there, not a fake pointer on a card.

Marshalling.  The launchers do not ask where their tensors live (the ``*_supported`` predicates do), so they run on small CPU tensors
against a stand-in for ``_lib.lib()`` that calls nothing and returns 0 (``recording``).  Per native call the symbol and every argument
are recorded (``normalise``): an integer as it is, a float as the float32 the library receives, a pointer as the label of the input
tensor it addresses (``x``, ``bias``, ... as the case names them; a derived operand the launcher keeps on the module under the names
the case gives it), ``new<i>`` for the i-th tensor the launcher allocated itself, ``null``."""
import contextlib
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PY = os.path.join(os.path.dirname(HERE), 'openpifpaf_amd', '_lib.py')
HIDE_GPUS = {'HIP_VISIBLE_DEVICES': '-1', 'ROCR_VISIBLE_DEVICES': '-1'}
P = 4096                                          # a fake device pointer (never dereferenced on the host)
I31 = 2 ** 31
OPA_ERR_HIP, OPA_ERR_WORKSPACE = 2, 4
STREAM = 0x7F00DEAD0040


def golden(name):
    return os.path.join(HERE, 'golden', name + '.json')


def assert_same(got, want):
    """The golden comparison: the same ids, and under every id the same record."""
    assert sorted(got) == sorted(want)
    different = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not different, different


def write_golden(path, document):
    """``document``: values of one line each, then the table -- one row per line: a difference reads as one line of a diff."""
    *head, (key, rows) = document.items()
    with open(path, 'w') as f:
        f.write('{' + ''.join('%s: %s,\n' % (json.dumps(k), json.dumps(v)) for k, v in head) + '%s: {\n' % json.dumps(key))
        f.write(',\n'.join('%s: %s' % (json.dumps(k), json.dumps(rows[k])) for k in sorted(rows)))
        f.write('\n}}\n')


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

class Entry:
    def __init__(self, table, symbol, tag='', **base):
        self.table, self.symbol, self.tag, self.base = table, symbol, tag, base

    def row(self, kind, **change):
        assert set(change) <= set(self.base), (self.symbol, change)
        args = [dict(self.base, **change)[k] for k in self.base]
        if self.symbol != 'opa_se_workspace_bytes':
            args.append(None)                                                            # the stream
        row_id = '%s%s(%s)' % (self.symbol, self.tag, ', '.join('%s=%s' % (k, 'null' if v is None else 'P+%d' % (v - P) if P < v < P + 16 else v)
                                                    for k, v in change.items()))
        assert row_id not in self.table, row_id
        self.table[row_id] = (kind, self.symbol, args)

    def refused(self, *changes, **also):
        for change in changes:
            self.row('refused', **dict(change, **also))

    def empty(self, *changes, **also):
        for change in changes:
            self.row('empty', **dict(change, **also))

    def each(self, names, values, **also):
        """Refused: every argument of ``names`` (one name or several) at every value of ``values``, one at a time."""
        for name in names.split():
            self.refused(*[{name: v} for v in values], **also)

    def null(self, names, **also):
        self.each(names, [None], **also)

    def off(self, names, by=(4, 8), **also):
        self.each(names, [P + d for d in by], **also)


def run_table(lib, table, canonical=None):
    """-> {row id: [status, message]} (``size`` rows: [the size, '']; the message of an OPA_OK is not read: success leaves it)."""
    out = {}
    for row_id, (kind, symbol, args) in table.items():
        status = getattr(lib, symbol)(*args)
        message = lib.opa_last_error().decode() if status != 0 and kind != 'size' else ''
        out[row_id] = [status, canonical(symbol, message) if canonical else message]
    return out


def child(table, canonical=None, also=None):
    """A test file's ``__main__``: runs its table and prints ``{(what ``also(lib)`` adds,) "rows": ...}``."""
    spec = importlib.util.spec_from_file_location('opa_lib', LIB_PY)                      # (the binding alone: no torch in this process)
    _lib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(_lib)
    lib = _lib.lib()
    if lib.opa_device_count() != 0:
        sys.exit('refusal table: %d GPU(s) visible with %r: not run' % (lib.opa_device_count(), HIDE_GPUS))
    json.dump(dict(also(lib) if also else {}, rows=run_table(lib, table, canonical)), sys.stdout)


def run_in_child(test_file):
    proc = subprocess.run([sys.executable, os.path.abspath(test_file)], env=dict(os.environ, **HIDE_GPUS), capture_output=True, text=True,
                          timeout=300)                                                    # (the script's directory leads its sys.path)
    assert proc.returncode == 0, (proc.stdout[-2000:], proc.stderr[-2000:])
    return json.loads(proc.stdout)


def check_kinds(table, got, statuses):
    """What a table promises of its own rows, whatever the golden file says.  No row reaches a launcher (on a machine without a GPU a
    row that slips past the checks answers OPA_ERR_HIP, "no ROCm-capable device is detected"): a ``refused`` row has a status of
    ``statuses`` and a message under the entry point's name, a ``workspace`` row OPA_ERR_WORKSPACE, an ``empty`` row OPA_OK.  Only a
    ``variant`` row -- a Winograd variant of diagnostic builds, past the checks -- is answered by the production launcher's dispatch,
    with hipErrorInvalidValue before any call that touches a device.  A ``size`` row records a size."""
    assert 0 not in statuses and OPA_ERR_HIP not in statuses
    for row_id, (kind, symbol, _) in table.items():
        status, message = got[row_id]
        if kind in ('refused', 'workspace'):
            assert status in (statuses if kind == 'refused' else {OPA_ERR_WORKSPACE}) and message.startswith(symbol + ': '), (row_id, status, message)
        elif kind == 'empty':
            assert status == 0, (row_id, status, message)
        elif kind == 'variant':
            assert status == OPA_ERR_HIP and message.endswith(': invalid argument'), (row_id, status, message)
        else:
            assert kind == 'size', (row_id, kind)


def refusals(test_file, table, statuses):
    """The table of ``test_file`` run in a child and checked (``check_kinds``) -> the document its golden file holds."""
    got = run_in_child(test_file)
    check_kinds(table, got['rows'], statuses)
    return got


# ---- launch marshalling -------------------------------------------------------------------------------------------------------------

class Recorder:
    """Stands in for the loaded library: every symbol of ``_lib.SYMBOLS`` is a function that records its arguments."""

    def __init__(self, symbols):
        self.symbols, self.calls = symbols, []

    def __getattr__(self, name):
        if name not in self.symbols:
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            if name == 'opa_se_workspace_bytes':                # (a size, not a status: csrc/se.hip)
                return args[0] * ((args[1] + 511) // 512) * args[2] * 8
            return 0
        return call


@contextlib.contextmanager
def recording():
    """-> the recorder in place of the library, a current stream with a known handle, the library reported as built."""
    import torch
    from openpifpaf_amd import _lib
    rec = Recorder(_lib.SYMBOLS)

    class Stream:
        cuda_stream = STREAM
    saved = _lib.lib, _lib.available, torch.cuda.current_stream
    _lib.lib, _lib.available, torch.cuda.current_stream = (lambda: rec), (lambda: True), (lambda *a: Stream())
    try:
        yield rec
    finally:
        _lib.lib, _lib.available, torch.cuda.current_stream = saved


def canonical_call(name, row):
    """``opa_gemm_unit_bias_act_f32x3`` and ``opa_dwconv_bias_act`` are the calls of ``opa_gemm_unit_act_f32x3`` without a residual
    and of ``opa_dwconv_act`` with the activation codes 0 / 1 (``csrc/capi_trunk.hip`` forwards them literally): a record of either
    is read as the record of its superset, so that the golden files hold ONE spelling of these launches."""
    if name == 'opa_gemm_unit_bias_act_f32x3':
        return ['opa_gemm_unit_act_f32x3', row[:6] + ['null', 0] + row[6:]]
    if name == 'opa_dwconv_bias_act':
        return ['opa_dwconv_act', row]
    return [name, row]


def normalise(calls, labels):
    """[(symbol, raw arguments)] -> [[symbol, [integers, floats and pointer labels]]]; ``labels``: {address: label}.
    ``ctypes.c_void_p`` objects and plain integers are read alike; a float argument (``ctypes.c_float``) is recorded as the float32
    the library receives."""
    from openpifpaf_amd import _lib
    labels = dict(labels)
    labels[STREAM] = 'stream'
    out = []
    for name, args in calls:
        argtypes = _lib.SYMBOLS[name][1]
        assert len(args) == len(argtypes), (name, len(args), len(argtypes))
        row = []
        for a, ty in zip(args, argtypes):
            a = a.value if isinstance(a, ctypes.c_void_p) else a
            if ty is ctypes.c_void_p:
                assert a is None or (isinstance(a, int) and a != 0), (name, a)
                row.append('null' if a is None else labels.setdefault(a, 'new%d' % sum(1 for v in labels.values() if v.startswith('new'))))
            elif ty is ctypes.c_float:
                assert isinstance(a, float), (name, a)
                row.append(ctypes.c_float(a).value)
            else:
                assert isinstance(a, int), (name, a)
                row.append(int(a))
        out.append(canonical_call(name, row))
    return out


def record_all(cases, check=None, before=None):
    """``cases``: {case id: (call, {label: input tensor}[, derived operands after the call -> {label: tensor} or None[,
    ``fused.X3_TERMS`` during the call]])} -> {case id: [[symbol, [arguments]], ...]}.  ``before(rec)`` runs in front of every call,
    ``check(case id, what the call returned)`` behind it."""
    import torch
    from openpifpaf_amd import fused
    result = {}
    saved_terms = fused.X3_TERMS
    try:
        with recording() as rec, torch.no_grad():
            for case_id, (call, tensors, *rest) in cases.items():
                derived, terms = (rest + [None, None])[:2]
                fused.X3_TERMS = saved_terms if terms is None else terms
                rec.calls = []
                if before is not None:
                    before(rec)
                kept = call()                                   # (kept: what the launcher allocated stays allocated while it is labelled)
                labels = dict(tensors, **(derived() if derived is not None else {}))
                addresses = {t.data_ptr(): label for label, t in labels.items()}
                assert len(addresses) == len(labels), case_id  # (no two operands of a case at one address)
                result[case_id] = normalise(rec.calls, addresses)
                if check is not None:
                    check(case_id, kept)
                del kept
    finally:
        fused.X3_TERMS = saved_terms
    return result


def marshalling(cases, path, **hooks):
    """``record_all(cases, **hooks)`` compared with the golden file at ``path`` -> what was recorded."""
    with open(path) as f:
        want = json.load(f)['cases']
    got = record_all(cases, **hooks)
    assert_same(got, want)
    return got
