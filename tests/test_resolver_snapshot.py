"""The resolver as a whole: every answer of i2c_backward_schedule / i2c_kernel_family over the grid of tools/resolver_snapshot.py
(model x dtype x inference x group_lanes x backward_mode x post_layout x cubature rule x T x B, per-trajectory parameters, both sides
of every 2 GiB bound, per-cell targets / temperatures beyond the 4 GiB window) equals tests/golden/resolver_abi9.npz, entry for entry.
The fixture is recorded output of the library as it was before Impl::resolve replaced the nine deciding functions; the resolver is
host code, the same source in the host simulation and in the device library, so both are held to the one table."""
import importlib.util
import os

import pytest

import hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("resolver_snapshot", os.path.join(ROOT, "tools", "resolver_snapshot.py"))
rs = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rs)


def _check(lib):
    want, got = rs.load_fixture(), rs.snapshot(lib)
    assert got["main"].size == 8 * 3 * 3 * 6 * 4 * 2 * 2 * 3 * 25 * 7  # the whole grid, not a thinned one
    diff = rs.differences(want, got)
    assert not diff, "the resolver's answers moved (first differing problems):\n" + "\n".join(diff)


def test_resolver_matches_the_snapshot_hostsim():
    _check(hostsim.load())


@pytest.mark.gpu
def test_resolver_matches_the_snapshot_device_library():
    """The device library answers from the same table (no kernel is launched)."""
    lib = rs.pkg.load_library()
    assert not lib.is_host_sim
    _check(lib)
