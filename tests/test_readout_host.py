"""The read-out entry points (csrc/sg_readout.hip) share one host prologue; without a device: a NULL batch is refused by each of them under
its OWN name, and sg_render_ex refuses an unknown flag bit before anything else."""
import ctypes as C

from softgrip_amd import native


def test_null_batch_is_refused_under_the_entry_points_own_name():
    L = native.lib()
    INV = native.SG_ERR_INVALID
    cam = (C.c_double * 7)(0, 0, 0, 1, 90, -30, 45)
    dummy = C.c_void_p(8)      # never dereferenced: the argument checks come first
    calls = {
        "sg_get_poses": lambda: L.sg_get_poses(None, None, 1, None, None, None, None, None),
        "sg_render": lambda: L.sg_render(None, cam, None, 1, 8, 8, None, None, None, None),
        "sg_render_ex": lambda: L.sg_render_ex(None, cam, None, 1, 8, 8, native.SG_RENDER_SKIN, None, None, None, None),
        "sg_get_contacts": lambda: L.sg_get_contacts(None, None, 1, 16, None, None, None, None, None, None),
        "sg_ray": lambda: L.sg_ray(None, None, 1, 1, dummy, dummy, None, None, 31, 0.0, 0, None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == INV, name
        msg = L.sg_last_error()
        assert msg.startswith(name.encode() + b":") and b"null batch" in msg, (name, msg)
    # an unknown flag bit: before the NULL batch, the NULL camera and the image size
    assert L.sg_render_ex(None, None, None, 0, 0, 0, native.SG_RENDER_SKIN | 2, None, None, None, None) == INV
    assert L.sg_last_error() == b"sg_render_ex: unknown flag bits"
