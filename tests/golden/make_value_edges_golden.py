"""Generate tests/golden/value_edges_ref.npz from the REFERENCE implementation.

Run where the reference tree is present:   python tests/golden/make_value_edges_golden.py

The frames of tests/value_edge_common.py (checksums that come out as 0x0000 and 0xFFFF, sums that need the second
fold step, odd tails of 0xFF, saturated frames whose exact sum passes 2^31) go through the compiled reference shim
(oracle/_ref/libnfref.so: Packet::update_checksums, the switch's forward data path, push_vlan / pop_vlan), one frame
at a time. Per frame and operation the file holds what the reference returned, the two checksum fields of its
output, the output's length and its 64-bit frame hash; for the update, which returns nothing, the status is the
oracle's, as in fuzz_ref.npz. The frames themselves are not stored: the builder remakes them, and `h_in` (the hash
of every input frame, in order) pins it. Recorded results only."""
from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import oracle  # noqa: E402
import value_edge_common as ve  # noqa: E402

def save_npz(path, arrays):
    """np.savez_compressed with fixed member dates, so that the file regenerates bit for bit."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def reference(op: str, f: bytes):
    """(what the reference returned, its output frame) for one operation."""
    if op == "upd":
        return oracle.update_frame(f)[1], oracle.ref_update_frame(f)
    if op == "fwd":
        out, fw = oracle.ref_l3_forward_frame(f, bytes(ve.NH_TABLE[1]))
        return fw, out
    out, ok, _ = oracle.ref_vlan_frame(f, ve.PUSH_OP if op == "push" else ve.POP_OP, len(f) + 4)
    return ok, out


def main():
    oracle.build()
    path = os.path.join(HERE, "value_edges_ref.npz")
    save_npz(path, ve.record(reference))
    print("value_edges_ref.npz:", len(ve.named_frames()), "frames,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
