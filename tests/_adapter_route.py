"""Which route produced an adapter container (openmvg_amd/adapter/mvgx_adapter_policy.hpp).

A replacement TU finishes a failing mvgx_* call with the host application's own reference code, so a parity test that compares
the adapter's container with the reference passes whether the device or that fallback produced it. `device_route` makes the
difference visible: inside the block MVGX_ON_DEVICE_ERROR=throw (a device failure becomes a failed call of the shim instead of a
quiet fallback), and on leaving it the library's counters must say that exactly `expect_pairs` image pairs came from the device,
none from the fallback, with no failing device call.

`expect_pairs` is computed by the test from the TU's routing rule, never read back from a counter:
  Matcher_Regions       every pair whose two views have the route's region type (empty images count)
  Cascade hashing       every pair whose image I has regions (the reference skips the others)
  Geometric filter      every pair of the putative container (finite precision, fewer than 2^20 matches per pair) whose views the
                        functor's model can use on the device (E / Eo: pinhole intrinsics on both views; angular: intrinsics on both)
  Guided matching       (guided_device, guided_host): the accepted device pairs go to the device when the regions are uint8 / float /
                        binary rows of a supported length, to the reference's Geometry_guided_matching otherwise
`guided` may be a callable evaluated when the block ends (the accepted pairs are known from the container only then)."""
import contextlib
import ctypes as C


def counters(lib, reset=False):
    """(device pairs, fallback pairs, device failures) of an adapter library; reset clears them afterwards"""
    out = (C.c_uint64 * 3)()
    lib.mvgx_adapter_counters(out, 1 if reset else 0)
    return int(out[0]), int(out[1]), int(out[2])


def guided_counters(lib, reset=False):
    """(pairs guided on the device, pairs guided by the reference's host code) of a geometric-filter adapter library"""
    out = (C.c_uint64 * 2)()
    lib.mvgx_adapter_guided_counters(out, 1 if reset else 0)
    return int(out[0]), int(out[1])


class Route:
    def __init__(self, expect_pairs, guided):
        self.expect_pairs = expect_pairs
        self.guided = guided
        self.seen = None
        self.seen_guided = None


@contextlib.contextmanager
def device_route(lib, expect_pairs, monkeypatch, guided=None):
    """the calls inside the block must run on the device path of `lib`, `expect_pairs` image pairs in all"""
    counters(lib, reset=True)
    if guided is not None:
        guided_counters(lib, reset=True)
    route = Route(int(expect_pairs), guided)
    with monkeypatch.context() as m:
        m.setenv("MVGX_ON_DEVICE_ERROR", "throw")
        yield route
    route.seen = counters(lib, reset=True)
    assert route.seen == (route.expect_pairs, 0, 0), \
        f"(device pairs, fallback pairs, device failures) = {route.seen}, expected ({route.expect_pairs}, 0, 0)"
    if guided is not None:
        want = tuple(int(v) for v in (guided() if callable(guided) else guided))
        route.seen_guided = guided_counters(lib, reset=True)
        assert route.seen_guided == want, f"(guided on the device, guided on the host) = {route.seen_guided}, expected {want}"

