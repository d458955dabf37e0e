"""CPU checks of the CASES of tests/test_prefilter_gpu.py (not of the library): every kernel organisation of csrc/prefilter.hip is met
by every dtype and order, and the tile shapes give full, several and ragged LDS tiles at every tile width -- by the dispatch of
launch_filter_t restated in that file.  A later change of the dispatch that moves a case off its kernel shows here, without a GPU."""
import test_prefilter_gpu as P


def test_every_organisation_meets_every_dtype_and_order():
    seen = {(c[0], c[2], c[3]) for c in P._organisation_cases()}
    for dt in P.DT:
        for order in range(2, 6 if dt == "f16" else 8):
            orgs = ("wave", "strided", "serial") if dt == "f64" else ("wave_full", "wave", "tile", "strided", "serial")     # (lean kernels: float math)
            for org in orgs:
                assert (org, dt, order) in seen, (org, dt, order)
    assert P.HORIZON == {2: 18, 3: 23, 4: 30, 5: 36, 6: 42, 7: 49}


def test_tile_shapes_cover_full_several_and_ragged_tiles():
    kinds = set()
    for (outer, n, inner), dt, order in P._tile_cases():
        tl = P.tile_lines(n, dt)
        tiles, ragged = -(-inner // tl), inner % tl != 0
        kinds.add((dt in ("bf16", "f16"), tl, "one" if tiles == 1 else "several", "ragged" if ragged else "full"))
    for wide, lines in ((False, (64, 32, 16)), (True, (128, 64, 32))):
        for tl in lines:
            assert (wide, tl, "several", "ragged") in kinds, (wide, tl, kinds)
            if tl == 128:                       # (inner = 64 and 70: one tile, half empty)
                assert (wide, tl, "one", "ragged") in kinds
            else:
                assert (wide, tl, "one", "full") in kinds or (wide, tl, "several", "full") in kinds, (wide, tl, kinds)
