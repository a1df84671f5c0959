"""CPU: the references of tests/fused_driver.py (what tests/test_gpu_fused_variants.py compares the fused kernels with) checked
without a GPU -- every declared path boundary, K value and planted extreme present in the inputs generated for each default size,
no case list empty, and numpy against a row-by-row Python loop at n = 1025 for every case of the four families.  (The driver's own
--self-check also computes the references at the other default sizes; the GPU runs do that anyway.)"""
import fused_driver


def test_references_check_themselves(capsys):
    fused_driver.self_check(sizes=[fused_driver.SLOW_N])
    out = capsys.readouterr().out
    for family in fused_driver.FAMILIES:
        assert f"{family}: n={fused_driver.SLOW_N} ok" in out
