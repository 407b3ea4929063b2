"""Counting the launches of one eager step on the host, for the training tests and the timing tools
(tools/mmoe_time.py, tools/ple_time.py): one per library entry point and per torch operator that is not a
view or an allocation, an approximation of the device's launch count."""
import torch

from rankops import ops

# launches per library call (the rest launch once); torch operators (exact names, overload included) that only
# make views, allocate or read metadata, so launch nothing
TWO_LAUNCHES = {"rk_gemm_wgrad": 2, "rk_gemm_wgrad_grouped": 2}
NO_LAUNCH = {"view.default", "_unsafe_view.default", "reshape.default", "slice.Tensor", "select.int", "detach.default",
             "alias.default", "empty.memory_format", "empty_like.default", "empty_strided.default",
             "as_strided.default", "expand.default", "squeeze.dim", "squeeze.default", "unsqueeze.default",
             "transpose.int", "permute.default", "t.default", "split.Tensor", "unbind.int", "is_same_size.default",
             "lift_fresh.default", "_sparse_coo_tensor_with_dims_and_tensors.default", "sym_size.int",
             "sym_stride.int", "sym_numel.default"}


class _CountingLib:
    def __init__(self, lib, names):
        self._lib, self._names = lib, names

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("rk_") or name.endswith("_floats") or name.endswith("_size"):
            return fn

        def call(*args):
            self._names.extend([name] * TWO_LAUNCHES.get(name, 1))
            return fn(*args)
        return call


def launches_of(step):
    """The launches of one eager call of `step`, counted on the host: every librankops entry point called
    (rk_gemm_wgrad and its grouped form count twice: partials and reduction) and every torch operator not
    named in NO_LAUNCH.  A host count, not a device trace: an operator is taken as one launch whatever it
    runs underneath, and a fill the library issues itself (the weight-gradient entries' memset for an empty
    reduction) is not seen.  It serves to compare list lengths between configurations; the list is printed
    so that every entry can be read.  A list of names in call order."""
    from torch.utils._python_dispatch import TorchDispatchMode
    names = []
    real = ops._lib.load

    class Ops(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = str(func).replace("aten.", "")
            if name not in NO_LAUNCH:
                names.append("torch:" + name)
            return func(*args, **(kwargs or {}))
    lib = _CountingLib(real(), names)
    ops._lib.load = lambda: lib
    try:
        with Ops():
            step()
    finally:
        ops._lib.load = real
    torch.cuda.synchronize()
    return names
