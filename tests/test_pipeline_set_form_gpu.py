"""h2r_pipeline_set_form forces the form of a pipelined modpow_public_key call, so that either form can be tested on any box whatever
its hardware queues.  Whatever the form, every in-field buffer is byte-equal to the one the stream-ordered h2r_modpow_public_key_batch
writes for the same inputs (x and n are read, and the witness written, by the call's own launches on the caller's stream), results equal
pow(), statuses agree, and h2r_pipeline_info reports the forced form."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

E = 65537


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    import halo2_rsa_amd
    return halo2_rsa_amd


_inputs = {}


def inputs(H, w, L, B):
    """Four calls' inputs and what the stream-ordered export writes for them: computed once per shape and batch, shared by the forms."""
    key = (w, L, B)
    if key not in _inputs:
        chip = H.BigIntChip(w, w * L)
        rng = random.Random(77 * L + B)
        ifs, _ = chip.in_field_layout()
        calls = []
        for k in range(4):
            N = [rng.getrandbits(w * L) | (1 << (w * L - 1)) | 1 for _ in range(B)]
            X = [rng.randrange(n) for n in N]
            big = (k * 7) % B if (B > 1 or k >= 2) else None           # (a batch of one: calls 2 and 3 are the x >= n element)
            if big is not None:
                X[big] = N[big] + (0 if k == 2 else 1)                  # x >= n (x == n in call 2): NOT_IN_FIELD, the witness is still written
                if X[big] >> (w * L):
                    X[big] = N[big]
            x, n = chip.assign_integer(X), chip.assign_integer(N)
            ref_if = torch.zeros(B * ifs, dtype=torch.uint8, device="cuda")
            res = chip.pow_mod_fixed_exp(x, E, n, want_trace=False, check_in_field=True, in_field_buf=ref_if)
            torch.cuda.synchronize()
            calls.append(dict(X=X, N=N, x=x, n=n, big=big, ref_if=ref_if, ref_out=res.value.limbs_dev.clone(), ref_status=res.status.clone()))
        _inputs[key] = (chip, calls)
    return _inputs[key]


# forced TWO_QUEUE at small, ragged batches, at 517 x RSA-2048 (the throughput chain build) and at 1,283 x RSA-1024 (the one-wave chain);
# AUTO: whatever the box's probe says; forced ONE_LAUNCH_STEP above 512: the step launch's witness role
CASES = [(64, 32, 1, "two_queue"), (64, 32, 5, "two_queue"), (64, 32, 67, "two_queue"), (64, 32, 517, "two_queue"), (64, 16, 1283, "two_queue"),
         (64, 32, 1, "auto"), (64, 32, 5, "auto"), (64, 32, 67, "auto"), (64, 32, 517, "auto"), (64, 16, 1283, "auto"),
         (64, 32, 515, "step")]


@pytest.mark.parametrize("w,L,B,form", CASES)
def test_in_field_witness_of_pipelined_calls(H, w, L, B, form):
    from halo2_rsa_amd import _lib
    chip, calls = inputs(H, w, L, B)
    pl = chip.pow_fixed_layout(E)
    ifs, _ = chip.in_field_layout()
    f = {"two_queue": _lib.H2R_PIPE_TWO_QUEUE, "auto": _lib.H2R_PIPE_AUTO, "step": _lib.H2R_PIPE_ONE_LAUNCH_STEP}[form]
    pipe = H.Pipeline(chip, depth=3, side_streams=2, form=f)
    if form == "two_queue":
        pi = pipe.info(B)
        assert pi.record_form == _lib.H2R_PIPE_TWO_QUEUE and pi.three_queues == 1
    if form == "step":
        pi = pipe.info(B)
        assert pi.record_form == _lib.H2R_PIPE_ONE_LAUNCH_STEP and pi.three_queues == 0
    assert H.lib().h2r_pipeline_set_form(pipe._p, _lib.H2R_PIPE_SIDE_STREAM) == H.H2R_E_SHAPE
    assert H.lib().h2r_pipeline_set_form(pipe._p, 17) == H.H2R_E_SHAPE
    assert H.lib().h2r_pipeline_set_form(None, _lib.H2R_PIPE_AUTO) == _lib.H2R_E_NULL
    sets = [dict(trace=torch.zeros(B * pl.elem_stride, dtype=torch.uint8, device="cuda"),
                 ws=torch.zeros(chip.workspace_bytes(B, pl.num_mul_mods), dtype=torch.uint8, device="cuda"),
                 out=torch.zeros((B, chip.num_limbs), dtype=chip.torch_dtype, device="cuda"),
                 status=torch.zeros(B, dtype=torch.uint8, device="cuda"),
                 in_field=torch.zeros(B * ifs, dtype=torch.uint8, device="cuda")) for _ in range(3)]
    seen = []
    for k, c in enumerate(calls):                                       # four calls rotate through three buffer sets
        s = sets[k % 3]
        s["in_field"].zero_()                                           # (call 3 reuses call 0's set: a witness left out would show either way)
        pipe.modpow_public_key(c["x"], E, c["n"], s["trace"], s["ws"], s["out"], s["status"], s["in_field"])
        # x and n are read, and the witness, the results and the statuses written, by the call's own launches on this stream
        seen.append((s["in_field"].clone(), s["out"].clone(), s["status"].clone()))
    pipe.join()
    torch.cuda.synchronize()
    for k, c in enumerate(calls):
        got_if, got_out, got_status = seen[k]
        assert torch.equal(got_status, c["ref_status"]), k
        st = got_status.cpu().numpy()
        want = np.zeros(B, dtype=np.uint8)
        if c["big"] is not None:
            want[c["big"]] = H.H2R_E_NOT_IN_FIELD
        assert np.array_equal(st, want), k
        assert torch.equal(got_if, c["ref_if"]), k
        ok = got_status == 0
        assert torch.equal(got_out[ok], c["ref_out"][ok]), k
        vals = H.AssignedInteger(got_out, w).to_big_uint()
        assert all(vals[i] == pow(c["X"][i], E, c["N"][i]) for i in range(B) if i != c["big"]), k
    pipe.close()
