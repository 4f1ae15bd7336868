"""The life cycle the six table classes share, on the CPU: a host query needs a commit, every
setter invalidates it, a rejected setter does not, and a handle closes once and answers NfcsError afterwards."""
import pytest

import netflow_amd as nf
from table_lifecycle_common import CASES, SETTERS, same


@pytest.fixture(params=CASES, ids=lambda c: c.cls.__name__)
def case(request):
    c = request.param()
    yield c
    c.close()


def test_a_host_query_needs_a_commit(case):
    with case.build() as t:
        case.host(t)
    with case.cls() as fresh:
        with pytest.raises(nf.NfcsError):
            case.host(fresh)
        assert fresh.commit() is fresh
        case.host(fresh)  # the empty table answers


@pytest.mark.parametrize("cls,setter", SETTERS, ids=lambda v: v if isinstance(v, str) else v.cls.__name__)
def test_each_setter_invalidates_the_commit(cls, setter):
    case = cls()
    try:
        with case.build() as t:
            case.host(t)
            assert case.setters[setter](t) is t
            with pytest.raises(nf.NfcsError):
                case.host(t)
            case.host(t.commit())
    finally:
        case.close()


def test_a_rejected_setter_leaves_the_commit(case):
    with case.build() as t:
        want = case.host(t)
        with pytest.raises(nf.NfcsError, match="invalid argument"):
            case.reject(t)
        assert same(case.host(t), want)


def test_the_changing_setter_changes_the_answer(case):
    """What the GPU test of the upload rules relies on."""
    with case.build() as t:
        old = case.host(t)
        case.change(t)
        assert not same(case.host(t.commit()), old)


def test_close_twice_and_the_context_manager(case):
    t = case.build()
    assert t.ptr
    t.close()
    assert t.ptr is None
    t.close()
    with case.build() as t:
        assert t.ptr
    assert t.ptr is None


def test_every_method_after_close_raises(case):
    t = case.build()
    t.close()
    calls = list(case.setters.values()) + [case.change, case.host] + list(case.after_close)
    for call in calls:
        with pytest.raises(nf.NfcsError):
            getattr(t, call)() if isinstance(call, str) else call(t)
