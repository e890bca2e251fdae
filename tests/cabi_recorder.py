"""Records the C-ABI calls of a forward and of its backward as two ordered lists (tests/test_gpu_chain_call_plans.py,
tools/gen_chain_call_plans.py).

Every entry of lavila_amd._cabi.SIGNATURES on the loaded library handle is wrapped through `monkeypatch.setattr`, except the
pure queries (QUERIES). A call is recorded as [name, arg, arg, ...]: integers and floats as they are, pointers as 'null' or
'ptr' (addresses differ from run to run; whether an operand is there does not)."""
import ctypes

QUERIES = ('lvl_version', 'lvl_last_error', 'lvl_workspace_floats')


def _is_pointer(argtype):
    return argtype is ctypes.c_void_p or argtype is ctypes.c_char_p or hasattr(argtype, 'contents')


def _argument(value, argtype):
    if _is_pointer(argtype):
        if value is None:
            return 'null'
        address = value.value if isinstance(value, ctypes.c_void_p) else value
        return 'ptr' if address else 'null'
    if isinstance(value, bool):
        return int(value)
    return value


class Recorder:
    def __init__(self, monkeypatch):
        from lavila_amd import _cabi as C
        self.forward, self.backward = [], []
        self._into = None
        handle = C.lib()
        for name, (_, argtypes) in C.SIGNATURES.items():
            if name in QUERIES:
                continue

            def wrap(*args, _f=getattr(handle, name), _n=name, _t=argtypes):
                if self._into is not None:
                    self._into.append([_n] + [_argument(a, t) for a, t in zip(args, _t)])
                return _f(*args)
            monkeypatch.setattr(handle, name, wrap)

    def begin(self):
        """A new pair of lists; calls from here on are forward calls."""
        self.forward, self.backward = [], []
        self._into = self.forward

    def phase_backward(self):
        self._into = self.backward

    def end(self):
        self._into = None
        return {'forward': self.forward, 'backward': self.backward}


def dump_plans(plans, path):
    """{case: {'forward': [...], 'backward': [...]}} as JSON: every distinct call once, the plans as lists of indices."""
    import json
    table, index = [], {}

    def code(call):
        key = json.dumps(call)
        if key not in index:
            index[key] = len(table)
            table.append(call)
        return index[key]
    packed = {case: {phase: [code(c) for c in calls] for phase, calls in plan.items()} for case, plan in plans.items()}
    with open(path, 'w') as f:
        f.write('{"calls": [\n' + ',\n'.join(json.dumps(c) for c in table) + '\n],\n"plans": {\n')
        f.write(',\n'.join(f'{json.dumps(case)}: {json.dumps(plan)}' for case, plan in packed.items()) + '\n}}\n')


def load_plans(path):
    import json
    with open(path) as f:
        data = json.load(f)
    return {case: {phase: [data['calls'][i] for i in idx] for phase, idx in plan.items()}
            for case, plan in data['plans'].items()}
