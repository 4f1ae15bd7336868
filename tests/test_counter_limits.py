"""CPU checks of the deny-counter cases of counter_limits_common.py: the hash, the table size, the
stripes and the port limit are parsed out of the sources and every claim a case makes about egress_acl_kernel's LDS
table is recomputed from them, so the cases cannot go stale silently when the hash changes; and the library's host
walks (egress_acl_host, egress_acl_items_host) equal the numpy model on every case of the GPU module."""
import os
import re
from collections import Counter

import numpy as np
import pytest

import netflow_amd as nf
import counter_limits_common as cl

ROOT = os.path.dirname(nf.HERE)
read = lambda *p: open(os.path.join(*p)).read()


@pytest.fixture(scope="module")
def src():
    return dict(kernels=read(nf.HERE, "csrc", "nfcs_kernels.hip"), internal=read(nf.HERE, "csrc", "nfcs_internal.h"),
                api=read(ROOT, "include", "nfcs.h"))


@pytest.fixture(scope="module")
def sets():
    s = {P: cl.deny_set(P) for P in cl.SETS}
    yield s
    for x in s.values():
        x.close()


def const(text, name):
    return int(re.search(rf"constexpr \w+ {name} = (\d+)u?;", text).group(1), 0)


def test_the_constants_are_the_sources(src):
    m = re.search(r"uint32_t h = \(port \* (0x[0-9A-Fa-f]+)u\) >> (\d+);", src["kernels"])
    assert m, "egress_acl_kernel's hash line changed: rebuild the cases of counter_limits_common.py from the new one"
    assert (int(m.group(1), 16), int(m.group(2))) == (cl.HASH_MUL, cl.HASH_SHIFT), "the hash changed: the cases are stale"
    assert "h = (h + 1u) & (kBlock - 1u)" in src["kernels"], "the probe step changed"
    k = src["internal"]
    assert const(k, "kWave") * const(k, "kWavesPerBlock") == cl.TABLE and "constexpr int kBlock = kWave * kWavesPerBlock;" in k
    assert const(k, "kCtAclStripes") == cl.STRIPES and const(k, "kCtLineSlots") == cl.LINE_SLOTS
    assert int(re.search(r"#define NFCS_L2_MAX_PORTS (\d+)u", src["api"]).group(1)) == cl.MAX_PORTS
    assert 32 - cl.HASH_SHIFT == 8 and 1 << 8 == cl.TABLE


def test_the_scratch_ends_with_port_1023_of_stripe_15(src):
    k = src["internal"]
    stripes = const(k, "kCtStripes")
    assert "kCtAclAt = 2u * kCtStripes * kCtLineSlots" in k and "kCtSlots = kCtAclAt + kCtAclStripes * 2u * NFCS_L2_MAX_PORTS" in k
    assert "return (2u * ports + kCtLineSlots - 1u) & ~(kCtLineSlots - 1u);" in k
    at = 2 * stripes * cl.LINE_SLOTS
    slots = at + cl.STRIPES * 2 * cl.MAX_PORTS
    assert at + cl.STRIPES * cl.acl_stride(cl.MAX_PORTS) == slots
    assert at + (cl.STRIPES - 1) * cl.acl_stride(1024) + 2 * 1023 + 1 == slots - 1  # the bytes of port 1023 in stripe 15
    # the four sets: one fold workgroup exactly, one slot pair more, a stride that is rounded up, the full extent
    assert [2 * P for P in cl.SETS] == [256, 258, 2046, 2048]
    assert [cl.acl_stride(P) for P in cl.SETS] == [256, 272, 2048, 2048]
    assert [(2 * P + cl.TABLE - 1) // cl.TABLE for P in cl.SETS] == [1, 2, 8, 8]


def test_why_the_older_tests_were_blind():
    """Ports 0..63 (ACL_PORTS = 37, L <= 64) fall into 64 buckets: no probe ever met another port's entry."""
    assert len({cl.bucket(p) for p in range(64)}) == 64
    assert cl.table_sim(range(64))[1:] == (0, 0)
    assert cl.first_colliding_pair() == (4, 148) and cl.bucket(4) == cl.bucket(148) == 120
    assert cl.fullest_bucket() == (63, [36, 180, 413, 646, 790, 1023])
    assert len(cl.wrapping_ports()) == 24


def tables(name, entry="plain"):
    return cl.workgroup_tables(cl.CASES[name], entry)


@pytest.mark.parametrize("name", [k for k in cl.CASES if k.startswith("pair")])
@pytest.mark.parametrize("entry", cl.ENTRIES)
def test_the_pair_collides_once(name, entry):
    (table, stepped, wrapped), = tables(name, entry)
    assert stepped == 1 and wrapped == 0 and sorted(table.values()) == [4, 148] and sorted(table) == [120, 121]
    first = {"pair in one wave": 4, "pair in two waves": 4, "pair in two waves, the later port first": 148}[name.rsplit("-", 1)[0]]
    assert int(cl.CASES[name]["port"][0]) == first


@pytest.mark.parametrize("entry", cl.ENTRIES)
def test_the_fullest_bucket_chains(entry):
    for name in ("fullest bucket, spread over the waves", "fullest bucket, all in every wave"):
        (table, stepped, wrapped), = tables(name, entry)
        assert sorted(table) == list(range(63, 69)) and stepped == 15 and wrapped == 0  # 0 + 1 + .. + 5 steps
    c = cl.CASES["fullest bucket, spread over the waves"]
    per_wave = [sorted(set(c["port"][w * 64:w * 64 + 64].tolist())) for w in range(4)]
    assert per_wave == [[36, 790], [180, 1023], [413], [646]]
    c = cl.CASES["fullest bucket, all in every wave"]
    assert all(len(set(c["port"][w * 64:w * 64 + 64].tolist())) == 6 for w in range(4))


@pytest.mark.parametrize("n", [256, 513])
@pytest.mark.parametrize("entry", cl.ENTRIES)
def test_the_probes_wrap(n, entry):
    t = tables(f"wrapping probes-{n}", entry)
    assert len(t) == (n + 255) // 256
    for table, stepped, wrapped in t[:n // 256]:
        assert len(table) == 24 and wrapped >= 1 and stepped > wrapped
        assert 255 in table and 0 in table and cl.bucket(table[0]) >= 250  # an entry below holds a port hashed above
    assert len(t[-1][0]) == (24 if n == 256 else 1)


@pytest.mark.parametrize("name", [k for k in cl.CASES if k.startswith("full table low") or k.startswith("full table high")])
@pytest.mark.parametrize("entry", cl.ENTRIES)
def test_the_table_is_full(name, entry):
    c, t = cl.CASES[name], tables(name, entry)
    for table, stepped, wrapped in t[:c["n"] // 256]:
        assert len(table) == 256 and sorted(table) == list(range(256)) and stepped > 0 and wrapped > 0
    if c["n"] % 256:
        assert len(t[-1][0]) == 1  # a last workgroup with one lane
    for lo in range(0, c["n"] - 63, 64):  # every lane of a full wave leads its own group
        assert len(set(c["port"][lo:lo + 64].tolist())) == 64
    assert int(c["port"].max()) == (1023 if "high" in name else 255)


@pytest.mark.parametrize("name", ["full table with the rest", "full table with the rest-1023"])
@pytest.mark.parametrize("entry", cl.ENTRIES)
def test_the_full_table_stands_beside_lanes_that_do_not_count(name, entry):
    c, m = cl.CASES[name], cl.model(cl.CASES[name], entry)
    t = cl.workgroup_tables(c, entry)
    # the mixed workgroups deny on three ports (an item without a source frame is not bypassed), two of them the pair
    assert [len(x[0]) for x in t] == [3, 256, 3] and t[1][2] > 0 and t[0][1] == 1
    for w in list(range(0, 4)) + list(range(8, 12)):  # every wave of the mixed workgroups holds every kind
        a = set(m["action"][w * 64:w * 64 + 64].tolist())
        assert a == {nf.ACL_DENY, nf.ACL_PERMIT, nf.ACL_NO_PORT, nf.ACL_BAD_DESC} | ({nf.ACL_BYPASS} if entry == "items" else set())
        p = c["port"][w * 64:w * 64 + 64]
        assert ((p >= c["P"]) & (p < cl.MAX_PORTS + 1)).any() and (p == 70000).any()


@pytest.mark.parametrize("P", [1024, 129])
def test_the_fold_cases(P):
    c = cl.CASES[f"fold-{P}"]
    assert c["n"] == 256 * cl.STRIPES * 2 + 1 and 2 * P > cl.TABLE  # every stripe twice; a fold of more than one workgroup
    m = cl.model(c, "plain")
    named = [0, 127, 128, 511, 1022, 1023] if P == 1024 else [127, 128]
    got = np.bincount(c["port"][m["denied"]], minlength=P)
    assert (got[named] > 256).all() and np.count_nonzero(got) == (206 if P == 1024 else 129)
    assert int(c["pk0"][P - 1]) == cl.PK1023 and int(m["pk"][P - 1]) < 1 << 16  # the last port's packets wrapped
    assert c["pk0"].all() and c["by0"].all()


@pytest.mark.parametrize("P", cl.SETS)
def test_every_port_of_every_set_counts(P):
    c = cl.CASES[f"every port-{P}"]
    m = cl.model(c, "items")
    got = np.bincount(c["port"][m["denied"]], minlength=P)
    assert got.all() and len(got) == P and m["action"].tolist().count(nf.ACL_BYPASS) > 100


@pytest.mark.parametrize("name", list(cl.CASES))
@pytest.mark.parametrize("entry", cl.ENTRIES)
def test_host_walks_equal_the_model(sets, name, entry):
    c = cl.CASES[name]
    m, h = cl.model(c, entry), cl.host(sets[c["P"]], c, entry)
    for k in ("action", "port", "pk", "by"):
        assert np.array_equal(h[k], m[k]), f"{k}: the host walk differs from the model"
    # a port swap inside a workgroup's table changes the byte counter when the two ports' byte sums there differ, and
    # the packet counter when their packet counts do
    pairs = same_by = same_pk = 0
    for w in cl.workgroup_sums(c, entry):
        v = list(w.values())
        pairs += len(v) * (len(v) - 1) // 2
        same_by += sum(x * (x - 1) // 2 for x in Counter(b for _, b in v).values())
        same_pk += sum(x * (x - 1) // 2 for x in Counter(k for k, _ in v).values())
    if name.startswith(("pair", "fullest", "wrapping", "full table")):
        assert same_by == 0, "two ports of one table have the same byte sum"  # every swap shows in the bytes
    else:  # fold, every port: up to 206 ports a workgroup on 90 lengths; the swaps the bytes cannot see stay under 1%
        assert same_by * 100 < pairs
    if name.startswith(("pair", "fullest")):
        assert same_pk == 0, "two ports of one table have the same packet count"  # and in the packets
    elif name.startswith("full table low") or name.startswith("full table high"):
        assert same_pk == pairs  # one packet per port, as the case is defined: only the bytes tell ports apart
