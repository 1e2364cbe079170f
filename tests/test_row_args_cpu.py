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


# ---------------------------------------------------------------------------------------------------- layout, rotary and step-cursor entries
ODD = BUF + 8              # 8-byte aligned only: a pointer the 16-byte vector loads and stores of these kernels cannot take


def rope(lib, batched, H=2, Ntok=4, T=0, B=1, buf=BUF, w=(BUF, BUF, BUF, BUF), cos=BUF, sin=BUF):
    tail = (0, 1e-6, None) if batched else (1e-6, None)
    f = lib.tfx_rmsnorm_rope_batched if batched else lib.tfx_rmsnorm_rope
    return f(buf, 1024, 4096, 0, 512, H, Ntok, T, B, *w, cos, sin, *tail)


@pytest.mark.parametrize("batched", (False, True))
def test_rmsnorm_rope_refuses_negative_extents_and_pointers_its_vector_loads_cannot_take(lib, batched):
    for kw in (dict(H=-1), dict(Ntok=-4), dict(B=-1), dict(T=-1)):              # a negative Ntok sized the grid from a negative count
        refused(lib, rope(lib, batched, **kw), b"negative H, Ntok, B or T")
    for kw in (dict(buf=ODD), dict(cos=ODD), dict(sin=ODD)) + tuple(dict(w=(BUF,) * i + (ODD,) + (BUF,) * (3 - i)) for i in range(4)):
        refused(lib, rope(lib, batched, **kw), b"16-byte aligned")
    assert rope(lib, batched, H=0) == 0 and rope(lib, batched, Ntok=0) == 0 and rope(lib, batched, B=0) == 0


def test_scatter_cols_and_copy_rows_refuse_negative_counts_and_unaligned_pointers(lib):
    scatter = lambda rows=4, src=BUF, dst=BUF: lib.tfx_scatter_cols(src, dst, rows, 64, 384, 64, None)
    copy = lambda rows=4, batch=2, src=BUF, dst=BUF: lib.tfx_copy_rows(src, 64, 512, dst, 384, 4096, rows, 64, batch, None)
    refused(lib, scatter(rows=-1), b"negative row count")
    refused(lib, scatter(src=ODD), b"16-byte aligned")
    refused(lib, scatter(dst=ODD), b"16-byte aligned")
    assert scatter(rows=0) == 0
    refused(lib, copy(rows=-1), b"negative row or batch count")
    refused(lib, copy(batch=-2), b"negative row or batch count")
    refused(lib, copy(src=ODD), b"16-byte aligned")
    refused(lib, copy(dst=ODD), b"16-byte aligned")
    assert copy(rows=0) == 0 and copy(batch=0) == 0


def test_unpack_latents_refuses_a_row_pitch_below_its_columns(lib):
    unpack = lambda ld, L=16, B=2: lib.tfx_unpack_latents(BUF, ld, BUF, B, 4, 6, L, 0.1159, 0.3611, None)
    for ld in (63, 56, 0, -64):
        refused(lib, unpack(ld), b"ld must be >= 4 L")
    assert unpack(64, B=0) == 0 and unpack(384, B=0) == 0


def test_transpose_refuses_a_batch_beyond_the_grid_and_pitches_below_the_extents(lib):
    tr = lambda N=100, C=72, batch=2, ldi=72, ldo=100: lib.tfx_transpose(BUF, ldi, 1 << 16, BUF, ldo, 1 << 16, N, C, batch, None)
    refused(lib, tr(batch=65536), b"batch must be <= 65535")
    refused(lib, tr(ldi=71), b"ldi must be >= C and ldo >= N")
    refused(lib, tr(ldo=99), b"ldi must be >= C and ldo >= N")
    assert tr(N=0) == 0 and tr(C=0) == 0 and tr(batch=0) == 0


def test_select_step_refuses_a_negative_size_and_unaligned_pointers(lib):
    sel = lambda per=64, table=BUF, cur=BUF, ptr=BUF: lib.tfx_select_step(table, cur, per, ptr, None)
    refused(lib, sel(per=-8), b"negative per-step size")
    refused(lib, sel(per=12), b"multiple of 8")
    refused(lib, sel(table=ODD), b"16-byte aligned")
    refused(lib, sel(cur=ODD), b"16-byte aligned")
    refused(lib, sel(ptr=BUF + 2), b"step_ptr 4-byte")
    assert sel(per=0) == 0 and sel(per=0, ptr=BUF + 4) == 0
