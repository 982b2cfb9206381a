"""GPU tests of the direct-light triple: k_logic evaluates it for the slots it gives the shadow bit, k_material only pushes those slots to the
shadow queue.  Against the CPU oracle on bits; set-ups and checks in direct_light_util.py, their slot-class preconditions established on the
oracle alone by test_direct_light_cpu.py and asserted again here.

Every test terminates for the reasons at the top of test_shade_edges_gpu.py: the crafted values only choose branches and stored values, and
the pre-filled directLight is read by one addition (logic.hlsl:230).
"""
import pytest

import direct_light_util as D
import shade_util as S

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def wide(monkeypatch):
    monkeypatch.setenv("GMUPT_TRAVERSAL", "wide")


@pytest.fixture(scope="module")
def scene(pkg):
    return S.edge_scene(pkg)


@pytest.fixture(scope="module")
def far_scene(pkg):
    return D.operand_scene(pkg)


def test_only_shadow_slots_rewrite_direct_light(pkg, device, scene):
    # a mid-flight pool: most slots retired by the path budget, the others crafted ended / UE4 with and without a shadow ray / glass in shuffled order
    c = D.Crafted(pkg, scene, S.block_layout(2), dev=device, path_budget=D.L + D.MIDFLIGHT_REFILL, max_depth=D.MIDFLIGHT_DEPTH)
    for k in "ESNGR":
        assert (c.kind == k).any(), "no slot of kind %s in the pool" % k
    D.check_direct_light(c.orc, c.hip, D.L, c.sent, c.kind, where="mid-flight pool: ")
    c.close()


@pytest.mark.parametrize("variant", [0, 1, 2], ids=["fixed", "mirror", "shuffle"])
def test_block_layouts(pkg, device, scene, variant):
    # blocks with no shadow-pushing slot, with nothing else, with a single one in the last lane, and the tail block cut by L
    c = D.Crafted(pkg, scene, S.block_layout(variant), dev=device)
    D.layout_preconditions(c.kind, variant)
    D.check_direct_light(c.orc, c.hip, D.L, c.sent, c.kind, where="layout %d: " % variant)
    c.compare(where="layout %d: " % variant)
    c.close()


@pytest.mark.parametrize("light_count", [1, D.MAX_LIGHTS])
def test_operand_identity(pkg, device, far_scene, light_count):
    # stored distance one ulp below the distance, light count 1 and the whole table, falloff below the distance, roughness 0, metallic 1,
    # NdotV <= 0, non-finite normal and throughput: directLight and the full state, after the shade group and after two more iterations
    c = D.Crafted(pkg, far_scene, D.operand_layout(), dev=device, light_count=light_count, far=True)
    D.operand_preconditions(c, light_count)
    D.check_direct_light(c.orc, c.hip, D.L, c.sent, c.kind, where="%d lights: " % light_count)
    c.compare(where="%d lights, shade group: " % light_count)
    c.casts()
    for it in range(2):
        c.step()
        c.compare(where="%d lights, iteration %d after: " % (light_count, it + 1))
    c.close()
