"""What the two image-tokenizer classes (vq.MAGVITv2, vqmodel.VQModel) share on the way to the `mmada_vq` handles of
libmmada_mi355x.so (csrc/vq_net.hip): building a handle from a state dict, the workspace, every run under the device the
weights live on, destroying the handles with the object, and reading a checkpoint directory."""
from __future__ import annotations

import ctypes as C
import fnmatch
import os
from typing import Dict, Iterable, Optional

import torch

from . import abi


def read_state_dict(root: str, bin_pattern: str, **load_kw) -> Dict[str, torch.Tensor]:
    """Every *.safetensors under `root`; without any, the files matching `bin_pattern` through torch.load(**load_kw)."""
    names = sorted(os.listdir(root))
    sd: Dict[str, torch.Tensor] = {}
    st_files = [f for f in names if f.endswith(".safetensors")]
    if st_files:
        from safetensors.torch import load_file

        for fn in st_files:
            sd.update(load_file(os.path.join(root, fn)))
        return sd
    bins = [f for f in names if fnmatch.fnmatchcase(f, bin_pattern)]
    if not bins:
        raise FileNotFoundError(f"no *.safetensors / {bin_pattern} under {root}")
    for fn in bins:
        sd.update(torch.load(os.path.join(root, fn), map_location="cpu", **load_kw))
    return sd


class VqHandles:
    """Base of MAGVITv2 and VQModel: owns their handles (up to one network per direction) and one workspace."""

    def __init__(self, what: str, device: Optional[torch.device]):
        if not torch.cuda.is_available():
            raise RuntimeError(f"{what} (MI355X) needs a GPU: there is no CPU fallback")
        self.device = torch.device(device if device is not None else "cuda:0")
        self._lib = abi.lib()
        self._handles = []
        self._ws = None

    def _build(self, create, what: str, create_args, state_dict, keys: Iterable[str], missing: str) -> C.c_void_p:
        """Handle from the library's create(*create_args, &handle) (`what` in its error) with state_dict[k] bound for every
        k of `keys`; KeyError("<n> <missing>") when the network expects tensors that `keys` did not bring."""
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            abi.check(create(*create_args, C.byref(h)), what)
            self._handles.append(h)
            st = abi.stream_ptr()
            for k in keys:
                t = state_dict[k].to(device=self.device, dtype=torch.float32).contiguous()
                abi.check(self._lib.mmada_vq_bind(h, k.encode(), t.data_ptr(), t.numel(), st), f"bind {k}")
            torch.cuda.current_stream().synchronize()  # the staged tensors `t` may be freed now
        n = self._lib.mmada_vq_num_unbound(h)
        if n:
            self._destroy(h)
            raise KeyError(f"{n} {missing}")
        return h

    def _workspace(self, handle, B: int, hz: int, wz: int):
        """(256-byte aligned device address, bytes) for a run of `handle` on a [B, hz, wz] latent grid; grows, never shrinks."""
        need = self._lib.mmada_vq_workspace_bytes(handle, B, hz, wz)
        if self._ws is None or self._ws.numel() < need + 256:
            self._ws = None
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        return (self._ws.data_ptr() + 255) // 256 * 256, need

    def _call(self, name: str, *args) -> None:
        """Library call `name`(*args, stream) on the current stream of the device the weights live on."""
        with torch.cuda.device(self.device):
            abi.check(getattr(self._lib, name)(*args, abi.stream_ptr()), name)

    def _destroy(self, h) -> None:
        self._handles.remove(h)
        self._lib.mmada_vq_destroy(h)

    def __del__(self):
        try:
            for h in list(getattr(self, "_handles", ())):
                self._destroy(h)
        except Exception:
            pass
