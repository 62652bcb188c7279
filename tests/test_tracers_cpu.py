"""The range of nscal (include/varden_amd.h: vdn_params): 1 .. 11, nscal + 5 <= VDN_MAXCOMP = 16 components of the bc tower (velocity, scalars,
pressure, extrap).  vdn_init checks the parameters before it looks for a device, so the refusal is the same with and without a GPU."""
import ctypes as C


def test_nscal_above_the_limit_is_refused_with_the_limit_named():
    from varden_amd import capi
    lib = capi.load()
    for bad in (12, 0):
        p = capi.default_params(nscal=bad)
        assert lib.vdn_init(C.byref(p), 0, 1, 0) != 0
        msg = lib.vdn_last_error()
        assert b"nscal = %d" % bad in msg and b"1..11" in msg and b"VDN_MAXCOMP = 16" in msg, msg
