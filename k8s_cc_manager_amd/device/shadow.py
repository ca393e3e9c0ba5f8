"""Shadow device backend: REAL GPU execution, shadowed mode registers.

Flipping SEV-SNP/TEE-IO GPU-CC state requires a privileged FLR/mode-1
reset that destroys every context on the device — on a shared GPU pool
that is not permissible. This backend is the honest middle tier used by
``bench.py`` and the GPU test suite (BASELINE.json config 4,
"devtools-equivalent mode with post-reset HIP attestation probe"):

- enumeration/identity come from the real HIP runtime (one
  :class:`ShadowHipDevice` per visible GPU, real PCI bdf);
- CC/fabric mode staging latches into an in-process shadow register
  with the same staged-until-reset semantics the hardware has;
- ``reset()`` applies the staged mode and invalidates "booted" state;
- ``wait_for_boot()`` is a REAL liveness gate: a kernel launch must
  round-trip on the device (``cc_device_alive``);
- the attestation probe (MFMA+LDS+HBM+xGMI) then runs for real.

So everything the framework would do around the privileged register
write is executed against real hardware; only the write itself is
shadowed. The privileged write path lives in
:mod:`.amdsmi_backend` behind ``CC_MANAGER_ALLOW_RESET``.
"""

from __future__ import annotations

import logging
import threading
from typing import List, Optional, Tuple

from .contract import (
    BootTimeoutError,
    CCDevice,
    CCDeviceError,
    DeviceBackend,
    FABRIC_OFF,
)

logger = logging.getLogger(__name__)


class ShadowHipDevice(CCDevice):
    def __init__(self, hip_index: int, bdf: str, name: str):
        self.hip_index = hip_index
        self.bdf = bdf
        self.name = name
        self._lock = threading.Lock()
        self._cc_mode = "off"
        self._fabric_mode = FABRIC_OFF
        self._staged_cc: Optional[str] = None
        self._staged_fabric: Optional[str] = None

    def is_gpu(self) -> bool:
        return True

    @property
    def cc_query_supported(self) -> bool:
        return True

    @property
    def fabric_query_supported(self) -> bool:
        return True

    def query_cc_mode(self) -> str:
        with self._lock:
            return self._cc_mode

    def set_cc_mode(self, mode: str) -> None:
        with self._lock:
            self._staged_cc = mode

    def query_fabric_mode(self) -> str:
        with self._lock:
            return self._fabric_mode

    def set_fabric_mode(self, mode: str) -> None:
        with self._lock:
            self._staged_fabric = mode

    def reset(self) -> None:
        with self._lock:
            if self._staged_cc is not None:
                self._cc_mode = self._staged_cc
                self._staged_cc = None
            if self._staged_fabric is not None:
                self._fabric_mode = self._staged_fabric
                self._staged_fabric = None

    def wait_for_boot(self, timeout: float = 60.0) -> None:
        from ..ops import attest

        try:
            rc = attest.device_alive(self.hip_index)
        except attest.AttestationError as e:
            raise CCDeviceError(str(e)) from e
        if rc != 0:
            raise BootTimeoutError(
                f"{self.bdf}: liveness kernel failed on HIP device "
                f"{self.hip_index} (rc={rc})"
            )


class ShadowBackend(DeviceBackend):
    """One ShadowHipDevice per visible GPU (optionally restricted)."""

    #: the mode register is an in-process shadow — never claim TEE
    #: enforcement (manager publishes ready.state=emulated, not true)
    hardware_backed = False

    def __init__(self, device_indices: Optional[List[int]] = None):
        from ..ops import attest

        n = attest.device_count()
        if n <= 0:
            raise CCDeviceError("no HIP devices visible")
        indices = device_indices if device_indices is not None else list(range(n))
        self._devices: List[ShadowHipDevice] = []
        for i in indices:
            bdf, name = _hip_identity(i)
            self._devices.append(ShadowHipDevice(i, bdf, name))

    def find_devices(self) -> Tuple[List[CCDevice], int]:
        return list(self._devices), len(self._devices)


def _hip_identity(index: int) -> Tuple[str, str]:
    """(bdf, name) for a HIP device, via torch when available (cheap)
    or amdsmi."""
    try:
        import torch

        props = torch.cuda.get_device_properties(index)
        bdf = f"{props.pci_domain_id:04x}:{props.pci_bus_id:02x}:{props.pci_device_id:02x}.0"
        return bdf, props.name
    except Exception:
        pass
    try:
        import amdsmi

        amdsmi.amdsmi_init()
        handles = amdsmi.amdsmi_get_processor_handles()
        h = handles[index]
        info = amdsmi.amdsmi_get_gpu_device_bdf(h)
        asic = amdsmi.amdsmi_get_gpu_asic_info(h)
        return str(info), asic.get("market_name", "AMD GPU")
    except Exception:
        return f"0000:00:{index:02x}.0", "AMD GPU (unidentified)"
