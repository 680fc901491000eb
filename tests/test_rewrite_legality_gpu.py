"""The fusion passes on graphs that are not the zoo's, on the kernels (MI355X).

test_rewrite_legality.py compares the fused program with the interpreter on the
CPU, where a fused op runs an fp32 torch reference of its folded parameters:
that never enters the HIP branch of the same op.  Here every device case of
rewrite_cases.py is compiled on the GPU with default_passes(), run once, and
compared with the fp64 value of the ORIGINAL graph under the kernels' own
bounds (rewrite_cases' references with gpu=True: kb.epilogue and its split-K
count, kb.post_output, kb.head_ref, kb.layernorm_ref, kb.attention_ref,
kb.softmax_ref, kb.dense_softmax_ref and the bit-exact kb.maxpool_ref; ops that
stay on torch get the bound of the arithmetic torch does).  The
broadcast-residual cases are the point: the CPU reference broadcasts a
[B,1,1,C] or [1,N] residual by itself, the kernels read one residual element
per output element.

A reference that chains two kernels through a stored intermediate it cannot
fetch (the QKV GEMM in front of the attention kernel) reads that intermediate
back from the program's own op, checks it against its own bound, and goes on
from the stored value.

The table's cases that stay off the device are those the passes leave to the
interpreter's torch ops entirely, or whose rewritten part is already run here
by a sibling case with the same fused ops (the link-by-link chain taps, the
leave-alone LayerNorm / pooling / conv variants, attention variants other than
the three here): their device programs run bf16 torch arithmetic for which
kernel_bounds has no derivation.

The `picks` fixture, `within` and the WORST table are test_fused_ops_gpu's: no
autotuning runs, and the worst err / bound per pass goes to FUSED_OPS_REPORT
with that module's op classes."""
import inspect
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import rewrite_cases as rc  # noqa: E402
import test_fused_ops_gpu as base  # noqa: E402  (the picks fixture, within, DEV and the report's WORST table)
import test_rewrite_legality as cpu  # noqa: E402  (check_histogram)
from rust_tensorflow_serving2_amd.graph import fused as FU  # noqa: E402

DEV, within, dev, picks = base.DEV, base.within, base.dev, base.picks
GEMM_OPS = ("_FusedConv2D", "_FusedMatMul", "_FusedQKV")     # (a _FusedDualConv whose sources only broadcast sums on torch)
DEVICE_CASES = [e for e in rc.CASES if e.gpu]


@pytest.mark.parametrize("entry", DEVICE_CASES, ids=lambda e: e.id)
def test_case_on_the_device(picks, monkeypatch, entry):
    from rust_tensorflow_serving2_amd.graph.compiler import compile_program
    from rust_tensorflow_serving2_amd.graph.ir import from_graph_def
    case = entry.build()
    prog = compile_program(from_graph_def(case.b.g.graph), case.b.feeds, case.fetches, device=DEV,
                           passes=FU.default_passes())
    cpu.check_histogram(case, prog.op_histogram(), gpu=True)
    outs = prog.run([dev(v) for v in case.b.inputs])
    torch.cuda.synchronize()
    if any(op in case.must_gpu for op in GEMM_OPS):
        assert picks.calls, "no GEMM launch went through ops.tuned_config: the HIP branch was not taken"
    monkeypatch.setattr(rc, "GPU_SPLITS", max([c["offered"][1] for c in picks.calls] or [1]))
    takes_prog = "prog" in inspect.signature(case.ref_gpu).parameters
    refs = case.ref_gpu(True, prog) if takes_prog else case.ref_gpu(True)
    assert len(refs) >= len(case.fetches)
    fam = "rewrite " + entry.group
    for name, y, (ref, bound) in zip(case.fetches, outs, refs):
        assert y.is_cuda, f"{name}: computed on the host"
        within(fam, y, ref, bound, f"{entry.id} {name}")
    for i, (y, ref, bound) in enumerate(refs[len(case.fetches):]):
        within(fam, y, ref, bound, f"{entry.id} stored intermediate {i}")


def test_device_only_passes_have_a_positive_control():
    """fuse_dual_conv and fuse_conv_chain rewrite on the device only (the
    opt-in fuse_matmul_layernorm and defer_layernorm are off by default)."""
    seen = set()
    for entry in DEVICE_CASES:
        seen |= set(entry.build().must_gpu)
    assert {"_FusedDualConv", "_ChainConv"} <= seen, seen


def test_zz_report_worst_ratios():
    """Not a check: writes the worst err / bound per op class and per pass when
    asked to (the other module's op classes included when it ran in the same session)."""
    path = os.environ.get("FUSED_OPS_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"worst": dict(sorted(base.WORST.items())), "rejected": base.REJECTED}, f, indent=1)
    assert all(v <= 1.0 for v in base.WORST.values())
