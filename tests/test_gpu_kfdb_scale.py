"""lld_kfdb_* on the scenes of tests/kfdb_scenes.py, where thousands of keyframes reach kfdb_score and kfdb_finish: up to 8192
kept entries (eight passes of the finish kernel's loops, every wavefront holding an accScore, a bitonic sort of up to 8192 keys),
hundreds of entries per de-duplication, 500 connected keyframes, BowVectors of up to 4000 words.  Every query must equal the
restatement tests/kfdb_ref.py with check(): ids in order, accScore bits, the four counters.  Each scene runs on two fresh handles
whose outputs must be bytewise equal, so the order of the atomics that fill `listed`, `kept` and `keys` does not show.  The
scenes all_retained[8192], groups and carry go on querying the used handle, against the restatement carried along."""
import pytest

import bow_ref as B
import kfdb_scenes as S
from lld_slam_amd import abi
from lld_slam_amd import vocabulary as voc
from lld_slam_amd.keyframe_database import KeyFrameDatabase

pytestmark = pytest.mark.gpu


def _vocab(gpu_ctx, seed, k):
    V = B.make_vocab(seed, k=k, L=4, p_full=1.0)
    return voc.ORBVocabulary.from_arrays(gpu_ctx, V["parent"], V["is_leaf"], V["desc"], V["weight"], V["k"], V["L"])


@pytest.fixture(scope="module")
def vocab(gpu_ctx):
    with _vocab(gpu_ctx, 41, 10) as v:                      # 10^4 words
        yield v


@pytest.fixture(scope="module")
def long_vocab(gpu_ctx):
    with _vocab(gpu_ctx, 42, 12) as v:                      # 12^4 words: room for 4000 words outside an 8000-word query
        yield v


def run_on_a_fresh_handle(v, sc, answers=None):
    """The scene on a new handle, each run of adds / erases / covisibility updates in one call.  With answers, every query is
    checked as it returns.  Returns per query (id bytes, accScore bytes, counters, full count)."""
    assert v.n_words == sc.n_words
    got, n = [], 0
    with KeyFrameDatabase(v, max_keyframes=sc.max_keyframes, max_words=sc.max_words) as dev:
        for op in S.batched(sc.ops):
            k = op[0]
            if k == "add_many":
                assert dev.add_raw(op[1], op[2]) == abi.LLD_OK
            elif k == "erase_many":
                assert dev.erase_raw(op[1]) == abi.LLD_OK
            elif k == "cov_many":
                assert dev.set_covisibles_raw(list(op[1]), list(op[1].values())) == abi.LLD_OK
            elif k == "clear":
                dev.clear()
            else:
                if k == "loop":
                    st, out, full = dev.detect_loop_candidates_raw(op[1], op[2], op[3], op[4])
                else:
                    st, out, full = dev.detect_relocalization_candidates_raw(op[1], op[2], capacity=op[3] if k == "reloc_cap" else None)
                assert st == abi.LLD_OK
                if answers is not None:
                    a = answers[n]
                    what = f"{sc.name} query {n}"
                    assert full == len(a.ids), what                       # the full count, whatever the capacity
                    cut = len(a.ids) if a.capacity is None else a.capacity
                    S.check(out, (a.ids[:cut], a.acc[:cut], a.stats), what)
                got.append((out.kf_id.tobytes(), out.acc_score.tobytes(), out.n_sharing, out.max_common_words, out.min_common_words,
                            out.n_scored, full))
                n += 1
    return got


@pytest.mark.parametrize("name", S.NAMES)
def test_scene_on_the_device(vocab, long_vocab, name):
    sc = S.scene(name)
    v = long_vocab if sc.n_words == S.LONG_N_WORDS else vocab
    answers = S.reference(name)
    first = run_on_a_fresh_handle(v, sc, answers)
    assert len(first) == len(answers)
    assert run_on_a_fresh_handle(v, sc) == first, f"{name}: two fresh handles differ"
