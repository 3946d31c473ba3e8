"""Code-generation properties of reverse_ldvi_kernel (cmcd_amd/csrc/cmcd_reverse_ldvi.hip), checked on the gfx950 ISA that hipcc
emits — no GPU needed, in the manner of tests/test_isa_reverse_uha.py.

  * Every network instance holds 4 T^2 fp32 matrix instructions: ONE copy of the step and ONE network evaluation per bridge (a
    peeled first iteration — m == K has no bridge to close — or a forward-kernel evaluation would change the count); the
    network-free instances hold none.
  * The instance list is exactly ldvi_traj_pick's eight.
  * Scratch is 0 wherever the ldvi_traj_kernel sibling has 0 (seven instances); the funnel instance on 5 neuron tiles, which spills
    100 bytes per lane in ldvi_traj_kernel, is held to the figure the compiler gives here, 28 (profiles/r21_reverse_ldvi_hais.txt
    records both).
  * Registers stay inside the launch bounds."""
import os

import pytest

from test_isa_properties import HIPCC, _asm, _kernel_whole, _scratch, _vgprs

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

GMM, FUNNEL, MANY = 0, 1, 2
KERNEL = "_ZN4cmcd19reverse_ldvi_kernelILi%dELi%dELi%dELb%dEEEvNS_15ReverseLdviArgsE"      # <TARGET, D, T, NET>
# ldvi_traj_pick's table: gmm / many_gmm (d = 2) on 2 and 4 neuron tiles, the funnel (d = 10) on 5, the three network-free ones
INSTANCES = [(t, 2, T, 1) for t in (GMM, MANY) for T in (2, 4)] + [(FUNNEL, 10, 5, 1)] + \
            [(GMM, 2, 1, 0), (MANY, 2, 1, 0), (FUNNEL, 10, 1, 0)]
SPILLS = {(FUNNEL, 10, 5, 1): 28}      # ldvi_traj_kernel<funnel, 10, 5, net>: 100


@pytest.fixture(scope="module")
def rev_asm(tmp_path_factory):
    from cmcd_amd import build
    assert "cmcd_reverse_ldvi.hip" in build.SOURCES
    return _asm(tmp_path_factory, "cmcd_reverse_ldvi.hip", build.EXTRA_FLAGS["cmcd_reverse_ldvi.hip"])


@pytest.mark.parametrize("inst", INSTANCES, ids=lambda i: "t%d_d%d_T%d_net%d" % i)
def test_every_instance_holds_one_copy_of_the_step(rev_asm, inst):
    body, tail = _kernel_whole(rev_asm, KERNEL % inst)
    _, D, T, net = inst
    mfma = sum("v_mfma_f32_16x16x4_f32" in l for l in body)
    print(inst, "mfma", mfma, "scratch", _scratch(tail), "vgprs", _vgprs(tail))
    assert mfma == (4 * T * T if net else 0), (inst, mfma)
    assert _scratch(tail) == SPILLS.get(inst, 0), (inst, _scratch(tail))
    # __launch_bounds__(512, (T > 4 || D > 4) ? 2 : 4): 256 / 128 registers
    assert _vgprs(tail) <= (128 if (T <= 4 and D <= 4) else 256), (inst, _vgprs(tail))


def test_the_table_is_the_forward_kernels(rev_asm):
    """exactly the eight instances of ldvi_traj_pick: no other instantiation in the file's device code"""
    names = {l.split(":")[0] for l in rev_asm if l.startswith("_ZN4cmcd19reverse_ldvi_kernel") and ":" in l}      # the function labels
    assert names == {KERNEL % i for i in INSTANCES}
