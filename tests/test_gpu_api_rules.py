"""The library's entry points refuse what they refused before their argument
rules moved to csrc/me_api_rules.cpp: tests/golden/api_args.json
(tests/golden/make_api_args.py) replayed through the built library on one
device.  Same status for every case; same me_last_error text for every case
but the frame-batch ones ("loose"), whose wordings were merged.  Every call is
refused by a rule, so nothing is launched; the buffers behind the pointers are
real all the same."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_api_args as T  # noqa: E402

pytestmark = pytest.mark.gpu


def test_entry_points_refuse_the_recorded_calls():
    lib, alloc = T.open_lib(), T.allocator()
    ctx = ctypes.c_void_p()
    assert lib.me_create(ctypes.byref(ctx), None, 0) == 0
    try:
        table = T.load_table()
        assert len(table) > 500
        for w in table:
            status, message = T.run(lib, ctx.value, w, alloc)
            assert status == w["status"], (w, status, message)
            if w["loose"]:
                assert message, w
            else:
                assert message == w["message"], (w, message)
    finally:
        lib.me_destroy(ctx)
