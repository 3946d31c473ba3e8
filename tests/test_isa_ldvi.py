"""Code-generation properties of the LDVI kernels (cmcd_amd/csrc/cmcd_ldvi.hip), checked on the gfx950 ISA that hipcc emits — no
GPU needed, in the manner of tests/test_isa_properties.py: the d = 2 instances of the forward chain keep z, rho, w and the key in
registers (no scratch) at the four waves per SIMD their launch bounds ask for; the network's second layer and the item kernel's
contractions over the particles are fp32 matrix instructions; no kernel of the file adds floats to memory atomically."""
import os

import pytest

from test_isa_properties import HIPCC, _asm, _kernel_whole, _scratch, _vgprs

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

GMM, FUNNEL, MANY = 0, 1, 2
TRAJ = "_ZN4cmcd16ldvi_traj_kernelILi%dELi%dELi%dELb%dEEEvNS_8LdviArgsE"            # <TARGET, D, T, NET>
ITEM = "_ZN4cmcd20ldvi_net_grad_kernelILi%dELi%dEEEvNS_8LdviArgsE"                  # <D, T>
SWEEP = "_ZN4cmcd17ldvi_sweep_kernelILi%dELi%dELb%dEEEvNS_8LdviArgsE"               # <TARGET, D, NET>
# the d = 2 instances of the forward chain: the network on 2 and 4 neuron tiles, and the network-free form (T = 1 stands for none)
TRAJ_D2 = [(t, 2, T, 1) for t in (GMM, MANY) for T in (2, 4)] + [(t, 2, 1, 0) for t in (GMM, MANY)]


@pytest.fixture(scope="module")
def ldvi_asm(tmp_path_factory):
    from cmcd_amd import build
    assert "cmcd_ldvi.hip" in build.SOURCES and build.EXTRA_FLAGS["cmcd_ldvi.hip"] == ["-fno-slp-vectorize"]
    return _asm(tmp_path_factory, "cmcd_ldvi.hip", build.EXTRA_FLAGS["cmcd_ldvi.hip"])


@pytest.mark.parametrize("inst", TRAJ_D2, ids=lambda i: "t%d_d%d_T%d_net%d" % i)
def test_forward_chain_d2_instances_use_no_scratch(ldvi_asm, inst):
    body, tail = _kernel_whole(ldvi_asm, TRAJ % inst)
    assert _scratch(tail) == 0, (inst, _scratch(tail))
    assert _vgprs(tail) <= 128, (inst, _vgprs(tail))          # four waves per SIMD (__launch_bounds__(512, 4))
    mfma = sum("v_mfma_f32_16x16x4_f32" in l for l in body)
    T, net = inst[2], inst[3]
    assert mfma == (4 * T * T if net else 0), (inst, mfma)    # ONE network evaluation per bridge: layer 2, 4 T^2 instructions


def test_funnel_and_gradient_instances_exist(ldvi_asm):
    for name in (TRAJ % (FUNNEL, 10, 5, 1), TRAJ % (FUNNEL, 10, 1, 0), ITEM % (2, 2), ITEM % (2, 4), ITEM % (10, 5)) + \
            tuple(SWEEP % (t, d, net) for t, d in ((GMM, 2), (MANY, 2), (FUNNEL, 10)) for net in (0, 1)):
        _kernel_whole(ldvi_asm, name)
    # the sweep is network-free: no matrix instruction in it; d = 2: no scratch
    for t in (GMM, MANY):
        for net in (0, 1):
            body, tail = _kernel_whole(ldvi_asm, SWEEP % (t, 2, net))
            assert not any("v_mfma" in l for l in body) and _scratch(tail) == 0


def test_item_kernel_contracts_on_the_matrix_cores(ldvi_asm):
    """T = 2, d = 2 per work item: layer 2 forward and its transpose (2 x 4 T^2) and, per k-step of four particles, the outer
    products dW2 (T^2), dW1[:2d] (T) and dW3 (T): 32 + 4 x 8 = 64."""
    body, tail = _kernel_whole(ldvi_asm, ITEM % (2, 2))
    assert sum("v_mfma_f32_16x16x4_f32" in l for l in body) == 64
    assert _scratch(tail) == 0


def test_no_float_atomics_anywhere(ldvi_asm):
    """Repeated calls return the same bits: every partial sum goes to a slot of its own with a plain store, none is added to
    memory (no global_atomic_add_f32 or any other vector memory atomic in the file's device code)."""
    assert not [l for l in ldvi_asm if ("global_atomic" in l or "flat_atomic" in l) and not l.lstrip().startswith((";", "."))]
    assert any("global_store_dword" in l for l in ldvi_asm)
