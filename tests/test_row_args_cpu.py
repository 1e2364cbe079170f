"""Arguments the row kernels' public entries accept and should not, without a GPU: every call below is refused on the host with a
tfx_last_error message before any HIP call (the pointers are never dereferenced), and empty extents return 0 without a launch -- on a
machine with no device a launch would come back as an error."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from textflux_amd import _lib as L
    L.build()
    return L.lib()


BUF = 1 << 20              # 16-byte aligned, never dereferenced


def refused(lib, rc, text):
    assert rc != 0 and text in lib.tfx_last_error(), (rc, lib.tfx_last_error())


def ln(lib, D, R=4, B=2):
    return lib.tfx_ln_modulate(BUF, 3072, 0, BUF, 3072, 0, BUF, BUF, 0, R, B, D, 1e-6, None)


def ln_split(lib, D, R=4, B=2, split=0, second=BUF):
    return lib.tfx_ln_modulate_split(BUF, 3072, 0, BUF, 3072, 0, BUF, BUF, second, second, split, 0, R, B, D, 1e-6, None)


def ln_fp8(lib, D, R=4, B=2):
    return lib.tfx_ln_modulate_fp8(BUF, 3072, 0, BUF, 3072, 0, BUF, 0, BUF, BUF, 0, R, B, D, 1e-6, None)


def layernorm(lib, D, rows=4):
    return lib.tfx_layernorm(BUF, 3072, BUF, 3072, BUF, BUF, rows, D, 1e-5, None)


@pytest.mark.parametrize("call", (ln, ln_split, ln_fp8, layernorm))
def test_layernorm_entries_refuse_a_row_length_the_kernel_cannot_take(lib, call):
    for D in (0, -8, 4, 12, 3080):
        refused(lib, call(lib, D), b"D must be a positive multiple of 8 and <= 3072")
    assert call(lib, 8, 0) == 0 and call(lib, 3072, 0) == 0                    # no rows: nothing to launch
    refused(lib, call(lib, 8, -1), b"negative")
    if call is not layernorm:
        assert call(lib, 8, 4, 0) == 0
        refused(lib, call(lib, 8, 4, -2), b"negative")


def test_split_modulation_checks_its_split_row(lib):
    refused(lib, ln_split(lib, 8, split=-1), b"split_row")
    refused(lib, ln_split(lib, 8, split=5), b"split_row")
    refused(lib, ln_split(lib, 8, split=1, second=None), b"second modulation")
    assert ln_split(lib, 8, R=0, split=0, second=None) == 0
    refused(lib, lib.tfx_ln_modulate_split(None, 8, 0, BUF, 8, 0, BUF, BUF, BUF, BUF, 0, 0, 1, 1, 8, 1e-6, None), b"null pointer")


def test_groupnorm_refuses_bad_groups_before_it_divides_by_them(lib):
    gn = lambda B, HW, C, groups: lib.tfx_groupnorm_nhwc(BUF, BUF, BUF, BUF, BUF, B, HW, C, groups, 1e-6, 1, None)
    for groups in (0, -1, -32):
        refused(lib, gn(2, 64, 128, groups), b"must be positive")
    refused(lib, gn(2, 64, 0, 32), b"must be positive")
    for C, groups in ((128, 65), (128, 48), (64, 32), (136, 34), (24, 2)):      # > 64 groups | C % groups | 2 per group | C / 8 does not divide 256, twice
        refused(lib, gn(2, 64, C, groups), b"unsupported C / groups")
    refused(lib, gn(-1, 64, 128, 32), b"groupnorm: B")
    refused(lib, gn(2, -64, 128, 32), b"groupnorm: B")
    refused(lib, gn(65536, 64, 128, 32), b"groupnorm: B")
    assert gn(0, 64, 128, 32) == 0 and gn(2, 0, 128, 32) == 0


def test_scheduler_steps_refuse_a_bad_channel_count_or_input_pitch(lib):
    euler = lambda C, ldxin, rows=4, xin=BUF: lib.tfx_euler_step(BUF, BUF, xin, ldxin, C, rows, BUF, None, 0, None)
    amo = lambda C, ldxin, rows=4, xin=BUF: lib.tfx_amo_step(BUF, BUF, xin, ldxin, C, rows, BUF, None, 0, BUF, None)
    for step in (euler, amo):
        for C in (0, -64, 12):
            refused(lib, step(C, 384), b"C must be a positive multiple of 8")
        for ld in (100, 380, 56, 0, -384):                                      # not 16-byte rows | narrower than the C columns written
            refused(lib, step(64, ld), b"ldxin")
        refused(lib, step(64, 384, rows=-1), b"negative row count")
        assert step(64, 384, rows=0) == 0 and step(64, 0, rows=0, xin=None) == 0


def test_text_encoder_helpers_refuse_what_they_cannot_index(lib):
    gather = lambda n, D, vocab: lib.tfx_gather_rows(BUF, BUF, BUF, n, D, vocab, None)
    for vocab in (0, -1):
        refused(lib, gather(4, 64, vocab), b"vocab must be positive")
    for D in (0, -8, 12):
        refused(lib, gather(4, D, 100), b"D must be a positive multiple of 8")
    assert gather(0, 64, 100) == 0
    refused(lib, lib.tfx_timestep_embedding(BUF, BUF, -1, None), b"negative n")
    assert lib.tfx_timestep_embedding(BUF, BUF, 0, None) == 0
    assert lib.tfx_rmsnorm(BUF, 0, 8, BUF, BUF, 8, 0, 8, 1e-6, None) == 0
    assert lib.tfx_mul_act(BUF, 8, BUF, 8, BUF, 8, 0, 8, 0, None) == 0
    assert lib.tfx_add_into_f32(BUF, BUF, 0, 0, None) == 0
    assert lib.tfx_row_softmax(BUF, 8, BUF, 8, 0, 8, 1.0, None) == 0
