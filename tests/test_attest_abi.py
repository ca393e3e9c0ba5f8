"""The C surface of libccattest.so against its Python declarations: the
three report structs byte for byte, and the binding table against the
functions the C API file defines. Loads on a CPU box, makes no GPU call."""

import ctypes
import re

import pytest

from k8s_cc_manager_amd.ops import attest
from k8s_cc_manager_amd.ops.build import SRC

pytestmark = pytest.mark.skipif(
    not attest._LIB_PATH.exists(), reason="libccattest.so not built"
)


@pytest.fixture(scope="module")
def lib():
    return ctypes.CDLL(str(attest._LIB_PATH))  # restype defaults to c_int


@pytest.mark.parametrize(
    "sizeof_fn,mirror,frozen",
    [
        ("cc_report_sizeof", attest._CReport, 504),
        ("cc_mx_report_sizeof", attest._CMxReport, 320),
        ("cc_sweep_report_sizeof", attest._CSweepReport, 392),
    ],
)
def test_report_struct_abi_parity(lib, sizeof_fn, mirror, frozen):
    """A ctypes mirror must match its C struct byte for byte (a drifted
    mirror reads fields from wrong offsets: silent garbage), and the
    layouts are frozen."""
    assert getattr(lib, sizeof_fn)() == ctypes.sizeof(mirror)
    assert ctypes.sizeof(mirror) == frozen


def test_binding_table_matches_the_c_api(lib):
    for name in attest._BINDINGS:
        assert hasattr(lib, name), name  # resolves in the library
    defined = set(re.findall(r"^(?:int|void) (cc_\w+)\(", SRC.read_text(), re.M))
    assert len(defined) >= 20
    assert defined == set(attest._BINDINGS)
