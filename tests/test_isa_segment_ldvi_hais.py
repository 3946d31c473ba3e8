"""Code-generation properties of segment_ldvi_kernel (cmcd_amd/csrc/cmcd_segment_ldvi.hip) and segment_hais_kernel
(cmcd_amd/csrc/cmcd_segment_hais.hip), checked on the gfx950 ISA that hipcc emits — no GPU needed, in the manner of
tests/test_isa_reverse_ldvi.py.  Matrix instructions, scratch and registers are counted, nothing else.

  * Every LDVI network instance holds 4 T^2 fp32 matrix instructions: ONE copy of the bridge with ONE network evaluation (a
    peeled first iteration — m == k0 closes no bridge — or a second copy of the bridge for k0 == 0 would change the count, and
    with it the bit-for-bit composition of segments, which rests on the cut being evaluated by the same machine code on both
    sides).  The network-free instances and the three UHA instances hold none.
  * The instance lists are exactly those of the forward kernels: ldvi_traj_pick's eight, tile_pick_plain's three.
  * Scratch is 0 wherever the forward sibling has 0; the LDVI funnel instance on 5 neuron tiles, which spills 100 bytes per lane in
    ldvi_traj_kernel, is held to the figure the compiler gives here, 20 (SPILLS; profiles/r22_segment_ldvi_hais.txt records both).
  * Registers stay inside the launch bounds' budget."""
import os

import pytest

from test_isa_properties import HIPCC, _asm, _kernel_whole, _scratch, _vgprs

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

GMM, FUNNEL, MANY = 0, 1, 2
LDVI = "_ZN4cmcd19segment_ldvi_kernelILi%dELi%dELi%dELb%dEEEvNS_15SegmentLdviArgsE"      # <TARGET, D, T, NET>
HAIS = "_ZN4cmcd19segment_hais_kernelILi%dELi%dEEEvNS_15SegmentHaisArgsE"                # <TARGET, D>
# ldvi_traj_pick's table: gmm / many_gmm (d = 2) on 2 and 4 neuron tiles, the funnel (d = 10) on 5, the three network-free ones
LDVI_INSTANCES = [(t, 2, T, 1) for t in (GMM, MANY) for T in (2, 4)] + [(FUNNEL, 10, 5, 1)] + \
                 [(GMM, 2, 1, 0), (MANY, 2, 1, 0), (FUNNEL, 10, 1, 0)]
HAIS_INSTANCES = [(GMM, 2), (FUNNEL, 10), (MANY, 2)]      # cmcd_hais.hip's three (tile_pick_plain)
SPILLS = {(FUNNEL, 10, 5, 1): 20}    # ldvi_traj_kernel<funnel, 10, 5, net>: 100


@pytest.fixture(scope="module")
def ldvi_asm(tmp_path_factory):
    from cmcd_amd import build
    assert "cmcd_segment_ldvi.hip" in build.SOURCES
    return _asm(tmp_path_factory, "cmcd_segment_ldvi.hip", build.EXTRA_FLAGS["cmcd_segment_ldvi.hip"])


@pytest.fixture(scope="module")
def hais_asm(tmp_path_factory):
    from cmcd_amd import build
    assert "cmcd_segment_hais.hip" in build.SOURCES
    return _asm(tmp_path_factory, "cmcd_segment_hais.hip", build.EXTRA_FLAGS["cmcd_segment_hais.hip"])


@pytest.mark.parametrize("inst", LDVI_INSTANCES, ids=lambda i: "t%d_d%d_T%d_net%d" % i)
def test_every_ldvi_instance_holds_one_copy_of_the_bridge(ldvi_asm, inst):
    body, tail = _kernel_whole(ldvi_asm, LDVI % inst)
    _, D, T, net = inst
    mfma = sum("v_mfma_f32_16x16x4_f32" in l for l in body)
    print(inst, "mfma", mfma, "scratch", _scratch(tail), "vgprs", _vgprs(tail))
    assert mfma == (4 * T * T if net else 0), (inst, mfma)
    assert _scratch(tail) == SPILLS.get(inst, 0), (inst, _scratch(tail))
    # __launch_bounds__(512, (T > 4 || D > 4) ? 2 : 4): 256 / 128 registers
    assert _vgprs(tail) <= (128 if (T <= 4 and D <= 4) else 256), (inst, _vgprs(tail))


@pytest.mark.parametrize("inst", HAIS_INSTANCES, ids=lambda i: "t%d_d%d" % i)
def test_every_uha_instance_is_scratch_free_and_without_matrix_instructions(hais_asm, inst):
    body, tail = _kernel_whole(hais_asm, HAIS % inst)
    mfma = sum("v_mfma" in l for l in body)
    print(inst, "mfma", mfma, "scratch", _scratch(tail), "vgprs", _vgprs(tail))
    assert mfma == 0, (inst, mfma)
    assert _scratch(tail) == 0, (inst, _scratch(tail))      # hais_traj_kernel: 0 on all three
    assert _vgprs(tail) <= 256, (inst, _vgprs(tail))        # __launch_bounds__(256): the whole register file of a lane


def test_the_tables_are_the_forward_kernels(ldvi_asm, hais_asm):
    """exactly the eight instances of ldvi_traj_pick and the three of cmcd_hais.hip: no other instantiation in the device code"""
    names = {l.split(":")[0] for l in ldvi_asm if l.startswith("_ZN4cmcd19segment_ldvi_kernel") and ":" in l}      # the function labels
    assert names == {LDVI % i for i in LDVI_INSTANCES}
    names = {l.split(":")[0] for l in hais_asm if l.startswith("_ZN4cmcd19segment_hais_kernel") and ":" in l}
    assert names == {HAIS % i for i in HAIS_INSTANCES}
