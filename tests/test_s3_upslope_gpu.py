"""Outlets and upslope cells at 40000 x 40000 G(seed=3) against d8_flow_accum, which is reference-verified at this size
(tests/test_s3_digests_gpu.py, like the engine's fill -> flat-resolved directions used here).  On these loop-free
directions, for EVERY outlet o the number of cells whose outlet is o must equal d8_flow_accum at o; outlet[outlet[c]] ==
outlet[c] for every cell; and the number of non-255 cells of d8_upslope_cells at the largest river's mouth must equal the
accumulation there.  No cell is sampled away: the histogram and the gathers run over all 1.6e9 cells, in row blocks."""
import pytest

pytestmark = pytest.mark.gpu

N = 40000
BLOCK = 2000


def test_s3_outlets_and_upslope_cells_agree_with_the_accumulation(rd):
    import torch

    n = N
    Z = torch.empty((n, n), dtype=torch.float32, device="cuda")
    rd.synth_dem_dev(Z, seed=3)
    rd.fill_depressions_dev(Z)
    dirs = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    rd.d8_flow_directions_dev(Z, -9999.0, dirs, flats=True)
    torch.cuda.synchronize()
    del Z
    torch.cuda.empty_cache()
    assert int((dirs == 0).sum().item()) == 0 and int((dirs > 8).sum().item()) == 0     # loop-free, all data (S3 digests)
    area = torch.empty((n, n), dtype=torch.float64, device="cuda")
    rd.d8_flow_accum_dev(dirs, area)
    outlet = torch.empty((n, n), dtype=torch.int32, device="cuda")                        # uint32 indices < 2^31 here
    rd.d8_outlets_dev(dirs, outlet)
    torch.cuda.synchronize()
    assert int((outlet < 0).sum().item()) == 0                                            # every cell has an outlet
    flat = outlet.view(-1)
    counts = torch.zeros(n * n, dtype=torch.int32, device="cuda")
    ones = torch.ones(BLOCK * n, dtype=torch.int32, device="cuda")
    not_idempotent = 0
    for y in range(0, n, BLOCK):
        idx = flat[y * n:(y + BLOCK) * n].long()
        counts.index_add_(0, idx, ones)
        not_idempotent += int((flat[idx] != flat[y * n:(y + BLOCK) * n]).sum().item())
        del idx
    del ones
    print("cells with outlet[outlet[c]] != outlet[c]:", not_idempotent)
    assert not_idempotent == 0
    wrong = n_outlets = stray = 0
    af = area.view(-1)
    for y in range(0, n, BLOCK):
        sl = slice(y * n, (y + BLOCK) * n)
        own = torch.arange(y * n, (y + BLOCK) * n, dtype=torch.int32, device="cuda")
        is_out = flat[sl] == own
        n_outlets += int(is_out.sum().item())
        wrong += int((is_out & (counts[sl].double() != af[sl])).sum().item())
        stray += int((~is_out & (counts[sl] != 0)).sum().item())
        del own, is_out
    print("outlets:", n_outlets, "with a count unlike d8_flow_accum:", wrong, "counts on cells that are no outlet:", stray)
    assert n_outlets > 0 and wrong == 0 and stray == 0
    del counts
    m = int(torch.argmax(af).item())
    amax = float(af[m].item())
    del area, af, outlet, flat
    torch.cuda.empty_cache()
    up = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    rd.d8_upslope_cells_dev(dirs, m % n, m // n, m % n, m // n, up)
    torch.cuda.synchronize()
    members = int((up != 255).sum().item())
    print("largest accumulation", amax, "at", (m % n, m // n), "upslope members", members)
    assert members == int(amax) and int((up == 2).sum().item()) == 1 and int(up.view(-1)[m].item()) == 2
    del up, dirs
    rd.release_workspace()
    torch.cuda.empty_cache()
