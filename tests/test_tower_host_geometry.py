"""CPU: the pure-arithmetic entry points of the tower and the CrossNets (csrc/mlp.hip, csrc/cross_tower.hip) -- the
workspace sizes callers allocate (tests/interaction_abi.py hands the kernels exactly that many floats), the ``_supported``
predicates, and the argument checks that return before any HIP call.  The expected values were recorded from the library
before these entry points were spread over several translation units; the grid crosses every branch of ``plan_wgrad``
(fewer than 64 rows, the slice search, the 16-slice cap, projection workgroups with and without spare CUs), the ``N`` and
``ld_w`` roundings of the slab, and the LDS limits of the CrossNet predicates.  No pointer is ever dereferenced: the
workspace functions read the descriptor's shapes only, and every rejected call returns on a host-side check."""
import ctypes

from helpers import GOLDEN_DIR  # noqa: F401  (path setup via conftest)

BATCHES = (0, 1, 63, 64, 1024, 4096)
# name -> ([(K, N) per layer], w_out)
TOWERS = {
    "deepfm": ([(39, 256), (256, 128)], True),              # 39 -> 256 -> 128 (-> 1: the projection w_out)
    "deepfm_n1": ([(39, 256), (256, 128), (128, 1)], True),  # the same with the last step as a layer of its own
    "wide3": ([(208, 400), (400, 400), (400, 400)], False),
    "one2048": ([(16, 2048)], False),
    "over512": ([(100, 600), (600, 64)], True),             # one layer wider than 512: off the fast bodies
}
CROSS_W = (16, 221, 512, 528)
MIX_ER = ((1, 1), (4, 32), (8, 64), (9, 1))
FAKE = 0x7F0000001000      # a 16-byte aligned address that nothing reads

EINVAL, ENOSUP, EALIGN = -1, -2, -3     # include/dctr.h


def make_mlp(L, layers, w_out=False, ptr=FAKE):
    m = L.Mlp()
    for i, (K, N) in enumerate(layers):
        ly = m.layer[i]
        ly.W = ly.bias = ly.h = ly.dh = ly.gW = ly.gbias = ptr
        ly.K, ly.N, ly.relu = K, N, 1
        ly.ld_w, ly.ld_h = (K + 3) // 4 * 4, (N + 3) // 4 * 4
    m.n_layers = len(layers)
    if w_out:
        m.w_out = m.g_w_out = ptr
    return m


def mix_layers(W, E, R, n_cross=1):
    return [(W, E * R + E), (E * R, E * R), (E * R, W)] * n_cross


def measure(L):
    """Every value of the grid, in a fixed order, from the loaded library."""
    lib = L.lib()
    out = {}
    for name, (layers, w_out) in TOWERS.items():
        m = make_mlp(L, layers, w_out)
        out["bwd_ws/" + name] = [lib.dctr_mlp_bwd_workspace_floats(ctypes.byref(m), B) for B in BATCHES]
        out["train_ws/" + name] = [lib.dctr_mlp_train_workspace_floats(ctypes.byref(m), B) for B in BATCHES]
    for W in CROSS_W:
        m = make_mlp(L, [(W, W)] * 2)
        out["mat_ws/%d" % W] = [lib.dctr_crossnet_mat_bwd_workspace_floats(ctypes.byref(m), B) for B in BATCHES]
        out["mat_ok/%d" % W] = [lib.dctr_crossnet_mat_supported(W, n) for n in (1, 2, 12, 13)]
        for E, R in MIX_ER:
            m = make_mlp(L, mix_layers(W, E, R))
            out["mix_ws/%d/%d/%d" % (W, E, R)] = [lib.dctr_crossnet_mix_bwd_workspace_floats(ctypes.byref(m), B)
                                                 for B in BATCHES]
            out["mix_ok/%d/%d/%d" % (W, E, R)] = [lib.dctr_crossnet_mix_supported(W, n, E, R) for n in (1, 4, 5)]
    return out


EXPECTED = {'bwd_ws/deepfm': [43520, 43520, 43520, 43520, 696320, 696320],
 'bwd_ws/deepfm_n1': [43528, 43528, 43528, 43528, 696448, 696448],
 'bwd_ws/one2048': [34816, 34816, 34816, 34816, 278528, 278528],
 'bwd_ws/over512': [99128, 99128, 99128, 99128, 793024, 793024],
 'bwd_ws/wide3': [404400, 404400, 404400, 404400, 808800, 808800],
 'mat_ok/16': [1, 1, 1, 0],
 'mat_ok/221': [1, 1, 1, 0],
 'mat_ok/512': [1, 1, 1, 0],
 'mat_ok/528': [0, 0, 0, 0],
 'mat_ws/16': [544, 544, 544, 544, 8704, 8704],
 'mat_ws/221': [99456, 99456, 99456, 99456, 795648, 795648],
 'mat_ws/512': [525312, 525312, 525312, 525312, 1050624, 1050624],
 'mat_ws/528': [558624, 558624, 558624, 558624, 1675872, 1675872],
 'mix_ok/16/1/1': [1, 1, 0],
 'mix_ok/16/4/32': [1, 1, 0],
 'mix_ok/16/8/64': [0, 0, 0],
 'mix_ok/16/9/1': [0, 0, 0],
 'mix_ok/221/1/1': [1, 1, 0],
 'mix_ok/221/4/32': [1, 1, 0],
 'mix_ok/221/8/64': [0, 0, 0],
 'mix_ok/221/9/1': [0, 0, 0],
 'mix_ok/512/1/1': [1, 1, 0],
 'mix_ok/512/4/32': [0, 0, 0],
 'mix_ok/512/8/64': [0, 0, 0],
 'mix_ok/512/9/1': [0, 0, 0],
 'mix_ok/528/1/1': [0, 0, 0],
 'mix_ok/528/4/32': [0, 0, 0],
 'mix_ok/528/8/64': [0, 0, 0],
 'mix_ok/528/9/1': [0, 0, 0],
 'mix_ws/16/1/1': [124, 124, 124, 124, 1984, 1984],
 'mix_ws/16/4/32': [20820, 20820, 20820, 20820, 333120, 333120],
 'mix_ws/16/8/64': [279704, 279704, 279704, 279704, 839112, 839112],
 'mix_ws/16/9/1': [636, 636, 636, 636, 10176, 10176],
 'mix_ws/221/1/1': [1568, 1568, 1568, 1568, 25088, 25088],
 'mix_ws/221/4/32': [74724, 74724, 74724, 74724, 747240, 747240],
 'mix_ws/221/8/64': [493032, 493032, 493032, 493032, 1479096, 2465160],
 'mix_ws/221/9/1': [7048, 7048, 7048, 7048, 112768, 112768],
 'mix_ws/512/1/1': [3596, 3596, 3596, 3596, 53940, 53940],
 'mix_ws/512/4/32': [150276, 150276, 150276, 150276, 751380, 751380],
 'mix_ws/512/8/64': [792072, 792072, 792072, 792072, 792072, 3960360],
 'mix_ws/512/9/1': [16012, 16012, 16012, 16012, 240180, 240180],
 'mix_ws/528/1/1': [3708, 3708, 3708, 3708, 48204, 48204],
 'mix_ws/528/4/32': [154452, 154452, 154452, 154452, 772260, 772260],
 'mix_ws/528/8/64': [808600, 808600, 808600, 808600, 808600, 808600],
 'mix_ws/528/9/1': [16508, 16508, 16508, 16508, 214604, 214604],
 'train_ws/deepfm': [43520, 43522, 43528, 43528, 696448, 696832],
 'train_ws/deepfm_n1': [43528, 43530, 43536, 43536, 696576, 696960],
 'train_ws/one2048': [34816, 34818, 34824, 34824, 278656, 279040],
 'train_ws/over512': [99128, 99130, 99136, 99136, 793152, 793536],
 'train_ws/wide3': [404400, 404402, 404408, 404408, 808928, 809312]}


def test_workspace_sizes_and_predicates_are_the_recorded_ones():
    from deepctr_torch._hip import lib as L
    got = measure(L)
    assert sorted(got) == sorted(EXPECTED)
    for key in EXPECTED:
        assert got[key] == EXPECTED[key], key


def rejections(L):
    """(name, return code) of calls that a host-side check turns away before anything touches the device."""
    lib = L.lib()
    P = FAKE
    tower = make_mlp(L, *TOWERS["deepfm"])
    wide = make_mlp(L, [(16, 2049)])
    cross = make_mlp(L, [(16, 16)] * 2)
    cross_wout = make_mlp(L, [(16, 16)] * 2, w_out=True)
    mix = make_mlp(L, mix_layers(16, 4, 32))
    mix_wout = make_mlp(L, mix_layers(16, 4, 32), w_out=True)
    r = ctypes.byref
    return [
        # null x
        ("mlp_fwd/null_x", lib.dctr_mlp_fwd(r(tower), None, 40, 64, P, None)),
        ("mlp_bwd/null_x", lib.dctr_mlp_bwd(r(tower), None, 40, 64, P, 1, P, 40, P, None)),
        ("mlp_train_step/null_x", lib.dctr_mlp_train_step(r(tower), None, 40, 64, None, None, None, P, P, P, P, P, P, 40, P,
                                                          0, None, None)),
        ("mlp_train_wgrad/null_x", lib.dctr_mlp_train_wgrad(r(tower), None, 40, 64, P, P, P, P, None, None)),
        ("mat_fwd/null_x", lib.dctr_crossnet_mat_fwd(r(cross), None, 16, 64, None)),
        ("mat_bwd/null_x", lib.dctr_crossnet_mat_bwd(r(cross), None, 16, 64, P, 16, P, 16, P, None)),
        ("mix_fwd/null_x", lib.dctr_crossnet_mix_fwd(r(mix), 4, 32, None, 16, 64, None)),
        ("mix_bwd/null_x", lib.dctr_crossnet_mix_bwd(r(mix), 4, 32, None, 16, 64, P, 16, P, 16, P, None)),
        # ld_x % 4 != 0
        ("mlp_fwd/ld_x", lib.dctr_mlp_fwd(r(tower), P, 41, 64, P, None)),
        ("mlp_train_step/ld_x", lib.dctr_mlp_train_step(r(tower), P, 41, 64, None, None, None, P, P, P, P, P, P, 40, P, 0,
                                                        None, None)),
        ("mlp_train_wgrad/ld_x", lib.dctr_mlp_train_wgrad(r(tower), P, 41, 64, P, P, P, P, None, None)),
        ("mat_fwd/ld_x", lib.dctr_crossnet_mat_fwd(r(cross), P, 18, 64, None)),
        ("mat_bwd/ld_x", lib.dctr_crossnet_mat_bwd(r(cross), P, 18, 64, P, 16, P, 16, P, None)),
        # a layer with N > 2048
        ("mlp_fwd/n2049", lib.dctr_mlp_fwd(r(wide), P, 16, 64, None, None)),
        ("mlp_bwd/n2049", lib.dctr_mlp_bwd(r(wide), P, 16, 64, P, 2052, P, 16, P, None)),
        ("mat_fwd/n2049", lib.dctr_crossnet_mat_fwd(r(wide), P, 16, 64, None)),
        ("mix_fwd/n2049", lib.dctr_crossnet_mix_fwd(r(wide), 4, 32, P, 16, 64, None)),
        ("bwd_ws/n2049", lib.dctr_mlp_bwd_workspace_floats(r(wide), 64)),
        # w_out on a CrossNet
        ("mat_fwd/w_out", lib.dctr_crossnet_mat_fwd(r(cross_wout), P, 16, 64, None)),
        ("mat_bwd/w_out", lib.dctr_crossnet_mat_bwd(r(cross_wout), P, 16, 64, P, 16, P, 16, P, None)),
        ("mix_fwd/w_out", lib.dctr_crossnet_mix_fwd(r(mix_wout), 4, 32, P, 16, 64, None)),
        ("mix_bwd/w_out", lib.dctr_crossnet_mix_bwd(r(mix_wout), 4, 32, P, 16, 64, P, 16, P, 16, P, None)),
    ]


REJECTED = [('mlp_fwd/null_x', -1), ('mlp_bwd/null_x', -1), ('mlp_train_step/null_x', -1), ('mlp_train_wgrad/null_x', -1),
 ('mat_fwd/null_x', -1), ('mat_bwd/null_x', -1), ('mix_fwd/null_x', -1), ('mix_bwd/null_x', -1), ('mlp_fwd/ld_x', -3),
 ('mlp_train_step/ld_x', -3), ('mlp_train_wgrad/ld_x', -3), ('mat_fwd/ld_x', -3), ('mat_bwd/ld_x', -3),
 ('mlp_fwd/n2049', -2), ('mlp_bwd/n2049', -2), ('mat_fwd/n2049', -2), ('mix_fwd/n2049', -2), ('bwd_ws/n2049', 0),
 ('mat_fwd/w_out', -1), ('mat_bwd/w_out', -1), ('mix_fwd/w_out', -1), ('mix_bwd/w_out', -1)]


def test_bad_arguments_are_rejected_on_the_host():
    from deepctr_torch._hip import lib as L
    assert rejections(L) == REJECTED
    codes = dict(REJECTED)
    assert codes["mlp_fwd/null_x"] == EINVAL and codes["mlp_fwd/ld_x"] == EALIGN and codes["mlp_fwd/n2049"] == ENOSUP

