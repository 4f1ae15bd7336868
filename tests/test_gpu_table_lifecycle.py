"""The upload rules the six table classes share, on the device, over a burst of two frames in a
1 KiB arena: upload needs a commit, the device call needs an upload, a setter and a commit leave the device copy
as it is, and the next upload replaces it. Every rejected call is rejected by argument checks, before a launch."""
import pytest

import netflow_amd as nf
from table_lifecycle_common import CASES, same

pytestmark = pytest.mark.gpu


@pytest.fixture(params=CASES, ids=lambda c: c.cls.__name__)
def case(request):
    c = request.param()
    yield c
    c.close()


def test_upload_semantics(engine, case):
    with case.build() as t:
        case.uploaded(engine)
        with pytest.raises(nf.NfcsError):
            case.device(engine, t)  # not uploaded
        old = case.host(t)
        t.upload(engine)
        assert same(case.device(engine, t), old)
        case.change(t)  # invalidates the commit, not the upload
        with pytest.raises(nf.NfcsError):
            case.host(t)
        with pytest.raises(nf.NfcsError):
            t.upload(engine)
        assert same(case.device(engine, t), old)
        new = case.host(t.commit())
        assert not same(new, old)
        assert same(case.device(engine, t), old)  # committed, not yet uploaded
        t.upload(engine)
        assert same(case.device(engine, t), new)
        t.upload(engine).upload(engine)  # twice in a row
        assert same(case.device(engine, t), new)


def test_upload_needs_a_commit(engine, case):
    with case.cls() as t:
        with pytest.raises(nf.NfcsError):
            t.upload(engine)


def test_a_fresh_object_after_close(engine, case):
    t = case.build().upload(engine)
    case.uploaded(engine)
    want = case.host(t)
    assert same(case.device(engine, t), want)
    t.close()
    with pytest.raises(nf.NfcsError):
        t.upload(engine)
    with pytest.raises(nf.NfcsError):
        case.device(engine, t)
    with case.build() as fresh:
        case.uploaded(engine)
        case.change(fresh)
        new = case.host(fresh.commit())
        assert same(case.device(engine, fresh.upload(engine)), new) and not same(new, want)
