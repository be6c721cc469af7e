"""CPU guard for the fused train steps' class hierarchy (trainer/fused.py and its
subclasses, wherever they live: trainer/sharded.py): every method a subclass of
FusedBPRTrainStep overrides accepts every call the base class's code makes on it — the
round-3 regression (`_prepare` called with the base's new `on` argument, a TypeError only
the GPU tests saw) fails here without a GPU. Checks the override signatures against the
base's, binds the exact argument lists the base class passes at its call sites, and holds
the base constructor to its one allocation hook."""
import ast
import inspect

import pytest

ALLOCATION_HOOK = '_allocate'


def _all_subclasses(cls):
    out = []
    for sub in cls.__subclasses__():
        out += [sub] + _all_subclasses(sub)
    return out


def _classes():
    """The base class and every subclass of it (importing fused.py imports them all)."""
    from recbole_amd.trainer.fused import FusedBPRTrainStep, ShardedBPRTrainStep
    subs = _all_subclasses(FusedBPRTrainStep)
    assert ShardedBPRTrainStep in subs
    return FusedBPRTrainStep, subs


def _overrides(base, sub):
    return {name: fn for name, fn in vars(sub).items()
            if callable(fn) and not name.startswith('__') and hasattr(base, name)}


def _class_node(cls):
    """The AST of a class, from the module it is defined in."""
    tree = ast.parse(open(inspect.getsourcefile(cls)).read())
    return next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls.__name__)


def test_overrides_accept_the_base_signature():
    base, subs = _classes()
    for sub in subs:
        for name, fn in _overrides(base, sub).items():
            bs, ss = inspect.signature(getattr(base, name)), inspect.signature(fn)
            for p in bs.parameters.values():
                if p.kind in (p.VAR_POSITIONAL, p.VAR_KEYWORD):
                    continue
                assert p.name in ss.parameters or any(
                    q.kind == q.VAR_KEYWORD for q in ss.parameters.values()), (name, p.name)
            # positional arity: whatever the base accepts positionally, the override must too
            npos = sum(1 for p in bs.parameters.values()
                       if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD))
            args = [object()] * npos
            try:
                ss.bind_partial(*args)
            except TypeError as e:
                pytest.fail(f'{sub.__name__}.{name}: {e}')


def _calls_on_self(tree, method):
    """(n positional args, keyword names) of every self.<method>(...) call in the tree."""
    out = []
    for node in ast.walk(tree):
        if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)
                and node.func.attr == method and isinstance(node.func.value, ast.Name)
                and node.func.value.id == 'self'):
            out.append((len(node.args), [k.arg for k in node.keywords]))
    return out


def test_base_call_sites_bind_to_the_overrides():
    base, subs = _classes()
    base_node = _class_node(base)
    for sub in subs:
        overrides = _overrides(base, sub)
        assert overrides, sub
        for name, fn in overrides.items():
            sig = inspect.signature(fn)
            for npos, kws in _calls_on_self(base_node, name):
                try:
                    sig.bind(object(), *([object()] * npos), **{k: object() for k in kws})
                except TypeError as e:
                    pytest.fail(f'base calls self.{name}({npos} positional, {kws}) on '
                                f'{sub.__name__}: {e}')


def test_base_constructor_calls_only_the_allocation_hook():
    """FusedBPRTrainStep.__init__ runs before a subclass's state exists: of the methods
    a subclass overrides it may call the documented allocation hook and nothing else."""
    base, subs = _classes()
    init = next(n for n in _class_node(base).body
                if isinstance(n, ast.FunctionDef) and n.name == '__init__')
    overridden = set()
    for sub in subs:
        overridden |= set(_overrides(base, sub))
    assert ALLOCATION_HOOK in overridden
    called = {name for name in overridden if _calls_on_self(init, name)}
    assert called == {ALLOCATION_HOOK}, called
    assert ALLOCATION_HOOK in (base.__doc__ or '')
