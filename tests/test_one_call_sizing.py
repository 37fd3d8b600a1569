"""The sizing arithmetic of the one-call route (cross_attention_renderer_amd.one_call: scenes per lattice buffer, scenes and rays per
call, the call ranges) on plain integers: no device.  The byte counts are stand-ins of the real ones' shape (a fixed part plus a part
per scene and ray; 2.5 GB of lattice per scene); every expected value is worked out by hand from the definitions."""
import pytest

from cross_attention_renderer_amd.one_call import call_ranges, call_size, scenes_per_lattice


def ws_bytes(nb, nr):
    return 4096 + nb * nr * 460_000


def pair_bytes(nb):
    return nb * 2_500_000_000


# (scenes, gs_cap, R, budget) -> (gs, rc)
SIZES = {
    # 4096 + 5 * 4800 * 460000 = 11 040 004 096 <= 10^12
    "fits": ((5, 5, 4800, 10**12), (5, 4800)),
    # 192 rays are 88 320 000 bytes per scene: 12 scenes 1 059 844 096, 6 scenes 529 924 096, 3 scenes 264 964 096 <= 300 000 000
    "scene_halving": ((12, 12, 192, 300_000_000), (3, 192)),
    # per ray (4096 + 4800 * 460000) / 4800 = 460000.853...; 2 * 10^9 / that = 4347.8 -> 4347 // 48 * 48 = 4320
    "ray_chunking": ((1, 1, 65536, 2_000_000_000), (1, 4320)),
}


@pytest.mark.parametrize("name", sorted(SIZES))
def test_scenes_and_rays_per_call(name):
    args, want = SIZES[name]
    scenes, gs_cap, R, budget = args
    assert call_size(scenes, gs_cap, R, ws_bytes, budget) == want


def test_scene_halving_goes_through_six():
    """12 -> 6 -> 3: the workspace of whole scenes is asked for at exactly these counts (once more for the ray decision)."""
    asked = []

    def counting(nb, nr):
        asked.append((nb, nr))
        return ws_bytes(nb, nr)
    assert call_size(12, 12, 192, counting, 300_000_000) == (3, 192)
    assert asked == [(12, 192), (6, 192), (3, 192), (3, 192)]


def test_a_budget_below_48_rays_is_refused():
    # 20 000 000 / 460000.853 = 43.5 rays -> 0 whole double tiles
    with pytest.raises(RuntimeError, match="cannot hold even 48 rays"):
        call_size(1, 1, 65536, ws_bytes, 20_000_000)


def test_scenes_per_lattice_buffer():
    # half of the usable bytes is 2 * 10^10: 12 scenes are 3 * 10^10, 6 scenes 1.5 * 10^10
    assert scenes_per_lattice(12, pair_bytes, 40_000_000_000) == 6
    # capped at two buffers of 4000 MiB: half is 4 194 304 000 < 5 * 10^9 (two scenes): 12 -> 6 -> 3 -> 2 -> 1
    assert scenes_per_lattice(12, pair_bytes, min(40_000_000_000, 2 * (4000 << 20))) == 1
    assert scenes_per_lattice(1, pair_bytes, 0) == 1


@pytest.mark.parametrize("scenes,R,gs,rc", [(*SIZES[k][0][::2], *SIZES[k][1]) for k in sorted(SIZES)] + [(5, 100, 2, 48), (5, 96, 2, 96)])
def test_call_ranges_tile_scenes_and_rays_exactly_once(scenes, R, gs, rc):
    """Every (scene, ray) lies in exactly one call; ray chunks start at multiples of rc, which is whole double tiles (48 rays) whenever
    the rays are chunked at all.  Two lattice groups (the second one ragged) cover what one group of all scenes covers."""
    assert rc == R or rc % 48 == 0
    for groups in ([(0, scenes)], [(0, scenes // 2 + 1), (scenes // 2 + 1, scenes)]):
        seen = {}
        for p0, p1 in groups:
            for s0, s1, r0, r1 in call_ranges(p0, p1, gs, R, rc):
                assert p0 <= s0 < s1 <= p1 and s1 - s0 <= gs and (s0 - p0) % gs == 0
                assert 0 <= r0 < r1 <= R and r0 % rc == 0 and r1 - r0 <= rc
                for s in range(s0, s1):
                    seen[s, r0] = seen.get((s, r0), 0) + 1
                    assert r1 == min(R, r0 + rc)
        assert seen == {(s, r0): 1 for s in range(scenes) for r0 in range(0, R, rc)}
