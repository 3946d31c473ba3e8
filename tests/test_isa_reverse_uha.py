"""Code-generation properties of reverse_uha_kernel (cmcd_amd/csrc/cmcd_reverse_uha.hip), checked on the gfx950 ISA that hipcc
emits — no GPU needed, in the manner of tests/test_isa_segment_uha.py.

  * The step exists ONCE in every instance: 2 x 4 T^2 fp32 matrix instructions, the two network evaluations of a bridge and no
    other (a peeled first iteration — m == K has no bridge to close — or a second copy of the step would change the count).
  * The 13 instances whose siblings (segment_uha_kernel, uha_traj_kernel) run without scratch run without scratch, inside the
    register budget of their launch bounds; the two funnel geffner instances that spill there are held to the figures the compiler
    gives here, recorded beside the sibling's in profiles/r19_reverse_uha.txt (T = 5: 124 bytes per lane against
    segment_uha_kernel's 148; T = 9: 1884 against 1840)."""
import os

import pytest

from test_isa_properties import HIPCC, _asm, _kernel_whole, _scratch, _vgprs

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

GMM, FUNNEL, MANY = 0, 1, 2
GEFFNER, DDS = 0, 1
KERNEL = "_ZN4cmcd18reverse_uha_kernelILi%dELi%dELi%dELi%dEEEvNS_14ReverseUhaArgsE"      # <TARGET, ARCH, D, T>
# uha_pick's table: gmm / many_gmm (d = 2) and funnel (d = 10); dds 64; geffner on 2 / 4 / 5 / 9 neuron tiles
INSTANCES = [(t, GEFFNER, d, T) for t, d in ((GMM, 2), (FUNNEL, 10), (MANY, 2)) for T in (2, 4, 5, 9)] + \
            [(t, DDS, d, 4) for t, d in ((GMM, 2), (FUNNEL, 10), (MANY, 2))]
SPILLS = {(FUNNEL, GEFFNER, 10, 5): 124, (FUNNEL, GEFFNER, 10, 9): 1884}


@pytest.fixture(scope="module")
def rev_asm(tmp_path_factory):
    from cmcd_amd import build
    assert "cmcd_reverse_uha.hip" in build.SOURCES
    return _asm(tmp_path_factory, "cmcd_reverse_uha.hip", build.EXTRA_FLAGS["cmcd_reverse_uha.hip"])


@pytest.mark.parametrize("inst", INSTANCES, ids=lambda i: "t%d_a%d_d%d_T%d" % i)
def test_every_instance_holds_one_copy_of_the_step(rev_asm, inst):
    body, tail = _kernel_whole(rev_asm, KERNEL % inst)
    T = inst[3]
    mfma = sum("v_mfma_f32_16x16x4_f32" in l for l in body)
    print(inst, "mfma", mfma, "scratch", _scratch(tail), "vgprs", _vgprs(tail))
    assert mfma == 2 * 4 * T * T, (inst, mfma)
    assert _scratch(tail) == SPILLS.get(inst, 0), (inst, _scratch(tail))
    # __launch_bounds__(512, (T > 4 || D > 4) ? 2 : 4): 256 / 128 registers; T = 5 at d = 2 asks for 2 and gets 3 waves (<= 168)
    budget = 128 if (T <= 4 and inst[2] <= 4) else (168 if inst[2] == 2 and T == 5 else 256)
    assert _vgprs(tail) <= budget, (inst, _vgprs(tail))


def test_the_table_is_the_forward_kernels(rev_asm):
    """exactly the 15 instances of uha_pick: no other instantiation in the file's device code"""
    names = {l.split(":")[0] for l in rev_asm if l.startswith("_ZN4cmcd18reverse_uha_kernel") and ":" in l}      # the function labels
    assert names == {KERNEL % i for i in INSTANCES}
