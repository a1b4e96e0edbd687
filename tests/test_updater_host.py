"""What wf_updater_create (csrc/updater.hip) refuses before it makes a device call.  No GPU."""
import ctypes

import pytest

from support import wlib  # noqa: F401

WF_ERR_INVALID = -1


def create(wlib, **fields):
    """wf_updater_create with a null communicator on a descriptor with the given fields: (status, handle, message)."""
    d = wlib.UpdaterDesc(ndofs=8, **fields)
    h = ctypes.c_void_p()
    rc = wlib.lib().wf_updater_create(None, ctypes.byref(d), ctypes.byref(h))
    return rc, h.value, wlib.lib().wf_last_error().decode()


@pytest.mark.parametrize("flags", [2, 4])
def test_unknown_flag_bits_are_refused(wlib, flags):
    """WF_UPDATER_INLINE is the one flag: any other bit (2 selected a second arrangement of the overlapped apply
    once) is WF_ERR_INVALID, with the value in the message and no handle."""
    rc, handle, msg = create(wlib, flags=flags)
    assert rc == WF_ERR_INVALID and not handle
    assert "flags" in msg and str(flags) in msg.split("flags")[-1], msg


def test_neighbours_need_a_communicator(wlib):
    """Refused on the host, before any device call: this passes on a machine without a GPU."""
    rc, handle, msg = create(wlib, num_send_neighbors=1)
    assert rc == WF_ERR_INVALID and not handle
    assert "without a communicator" in msg, msg
