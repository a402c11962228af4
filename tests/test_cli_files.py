"""What the command-line tools (python -m flowonthego_amd.<tool>) do with the files they are given, before anything reaches the
device (no GPU needed): a file that is missing, is no file of its kind, or has another size or type than the tool needs ends the
tool with return value 1 and one line "<tool>: ..." on stderr that names the file and the sizes it should have had -- never with a
traceback.  The sequence tools' frame counts, their (T, h, w, 1) form and the context each builds for its frames are pinned with
a stand-in for OFClass, which stops the tool where the device would come in.  Every main(argv) is called in this process."""
import importlib
import os
import re

import numpy as np
import pytest

from host_checks import gray_png_bytes

H, W = 6, 9                   # the flow's size; the files "of another size" are (H + 1, W + 1)
SH, SW = 48, 64               # the sequences' frame size


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> path of every file the cases use; written once, read only"""
    from flowonthego_amd.flo import write_flo
    d = tmp_path_factory.mktemp("cli_files")
    rng = np.random.default_rng(3)
    p = {}

    def put(name, writer, *a):
        p[name.split(".")[0]] = str(d / name)
        writer(str(d / name), *a)

    def raw(path, data):
        open(path, "wb").write(data)

    img = rng.integers(0, 256, (H, W), dtype=np.uint8)
    big = rng.integers(0, 256, (H + 1, W + 1), dtype=np.uint8)
    put("flow.flo", write_flo, rng.standard_normal((H, W, 2)).astype(np.float32))
    put("flow_o.flo", write_flo, rng.standard_normal((H + 1, W + 1, 2)).astype(np.float32))
    put("mask.png", raw, gray_png_bytes(img))
    put("mask_o.png", raw, gray_png_bytes(big))
    put("mask_txt.png", raw, b"not a PNG at all\n")
    put("mask_cut.png", raw, gray_png_bytes(img)[:60])              # the file ends inside its data stream
    put("mask_short.png", raw, gray_png_bytes(img, rows=H - 2))     # a complete stream that holds too few rows
    put("gray.npy", np.save, img)
    put("gray_o.npy", np.save, big)
    put("gray_i16.npy", np.save, img.astype(np.int16))
    put("gray_f32.npy", np.save, img.astype(np.float32))
    put("ids.npy", np.save, np.zeros((H, W), np.int32))
    put("ids_i64.npy", np.save, np.zeros((H, W), np.int64))
    put("pts.npy", np.save, np.zeros((5, 2), np.float32))
    put("pts3.npy", np.save, np.zeros((5, 3), np.float32))
    seq = rng.integers(0, 256, (4, SH, SW, 3), dtype=np.uint8)
    put("seq.npy", np.save, seq[..., 0])
    put("seq_c1.npy", np.save, seq[..., :1])
    put("seq_rgb.npy", np.save, seq)
    put("seq_rgb_f32.npy", np.save, seq.astype(np.float32))
    for n in (0, 1, 2, 3):
        put("seq_%d.npy" % n, np.save, seq[:n, ..., 0])
    put("seq_i16.npy", np.save, seq[..., 0].astype(np.int16))
    put("seq_2d.npy", np.save, seq[0, ..., 0])
    put("seq_o.npy", np.save, seq[:, :, :SW - 4, 0])
    for name in ("none.flo", "none.npy", "none.png", "out.flo", "out.npy", "out.npz", "out.png", "traj.npy"):
        p[name.replace(".", "_")] = str(d / name)
    assert not any(os.path.exists(p[k]) for k in ("none_flo", "none_npy", "none_png"))
    return p


def run(tool, argv, files, capsys):
    """main(argv) of the tool with the file names filled in: (return value, stderr); nothing may go to stdout"""
    main = importlib.import_module("flowonthego_amd." + tool).main
    rc = main([a.format(**files) for a in argv])
    cap = capsys.readouterr()
    assert cap.out == ""
    return rc, cap.err


def refused(tool, argv, files, capsys, named=(), numbers=()):
    """return value 1, one line "<tool>: ..." without a traceback that names the files and, apart from them, holds the numbers"""
    rc, err = run(tool, argv, files, capsys)
    assert rc == 1, (tool, argv, err)
    assert err.startswith(tool + ": ") and err.endswith("\n") and err.count("\n") == 1 and "Traceback" not in err, err
    for k in named:
        assert files[k] in err, (k, err)
    rest = err
    for path in sorted(files.values(), key=len, reverse=True):
        rest = rest.replace(path, "")
    for n in numbers:
        assert re.search(r"(?<!\d)%d(?!\d)" % n, rest), (n, err)


# tool -> (its arguments with every input valid, the names of its input files among them)
VALID = {
    "fit_motion": (["{flow}", "--mask", "{mask}"], ("flow", "mask")),
    "moving_objects": (["{flow}", "--mask", "{mask}"], ("flow", "mask")),
    "motion_histograms": (["{flow}", "{out_npz}", "--mask", "{mask}", "--ids", "{ids}"], ("flow", "mask", "ids")),
    "motion_blur": (["{gray}", "{flow}", "{out_png}", "--mask", "{mask}"], ("gray", "flow", "mask")),
    "fb_check": (["{flow}", "{flow}", "{out_png}"], ("flow",)),
    "filter_flow": (["{flow}", "{gray}", "{out_flo}", "--bw", "{flow}"], ("flow", "gray")),
    "block_motion": (["{gray}", "{gray}", "{flow}", "{out_npz}", "--bw", "{flow}"], ("gray", "flow")),
    "chain_flow": (["{flow}", "{flow}", "{out_flo}", "--bw", "{flow}", "{flow}", "--points", "{pts}", "{traj_npy}"], ("flow", "pts")),
    "warp_frame": (["{gray}", "{gray}", "{flow}", "{out_png}", "--occ", "{gray}"], ("gray", "flow")),
    "interp_frame": (["{gray}", "{gray}", "0.5", "{out_png}", "--ref", "{gray}"], ("gray",)),
    "stabilize": (["{seq}", "{out_npy}"], ("seq",)),
    "track_objects": (["{seq}", "{out_npz}"], ("seq",)),
    "denoise": (["{seq}", "{out_npy}", "--ref", "{seq}"], ("seq",)),
}
assert len(VALID) == 13


def _missing_cases():
    """every input slot of every tool in turn holds the name of a file that does not exist, the other slots stay valid"""
    out = []
    for tool, (argv, inputs) in VALID.items():
        for i, a in enumerate(argv):
            if a.strip("{}") in inputs:
                gone = "none_" + ("flo" if a == "{flow}" else "png" if a == "{mask}" else "npy")
                out.append(pytest.param(tool, argv[:i] + ["{%s}" % gone] + argv[i + 1:], gone, id="%s-%d" % (tool, i)))
    out.append(pytest.param("motion_blur", ["{none_npy}", "{out_npy}"], "none_npy", id="motion_blur-sequence"))
    return out


@pytest.mark.parametrize("tool,argv,gone", _missing_cases())
def test_a_missing_input_file(tool, argv, gone, files, capsys):
    refused(tool, argv, files, capsys, named=(gone,))


MASK_TOOLS = {"fit_motion": ["{flow}"], "moving_objects": ["{flow}"], "motion_histograms": ["{flow}", "{out_npz}"],
              "motion_blur": ["{gray}", "{flow}", "{out_png}"]}


@pytest.mark.parametrize("tool", sorted(MASK_TOOLS))
def test_a_mask_png_the_tool_cannot_use(tool, files, capsys):
    head = MASK_TOOLS[tool]
    refused(tool, head + ["--mask", "{mask_o}"], files, capsys, named=("mask_o",), numbers=(W + 1, H + 1, W, H))
    refused(tool, head + ["--mask", "{mask_txt}"], files, capsys, named=("mask_txt",))
    refused(tool, head + ["--mask", "{mask_short}"], files, capsys, named=("mask_short",))
    # (a file that ends inside its data stream: what the decompressor says of it does not name the file)
    refused(tool, head + ["--mask", "{mask_cut}"], files, capsys)
    # an 8-bit RGB PNG is no mask either
    from flowonthego_amd.color import write_png
    write_png(files["out_png"], np.zeros((H, W, 3), np.uint8))
    refused(tool, head + ["--mask", "{out_png}"], files, capsys, named=("out_png",))
    os.remove(files["out_png"])


def test_a_backward_flow_of_another_size(files, capsys):
    for tool, argv in (("fb_check", ["{flow}", "{flow_o}", "{out_png}"]),
                       ("filter_flow", ["{flow}", "{gray}", "{out_flo}", "--bw", "{flow_o}"]),
                       ("block_motion", ["{gray}", "{gray}", "{flow}", "{out_npz}", "--bw", "{flow_o}"])):
        refused(tool, argv, files, capsys, named=("flow_o", "flow"), numbers=(W + 1, H + 1, W, H))
    # chain_flow names the first flow and its size, which every other flow must have: a forward and a backward flow that differ
    for argv in (["{flow}", "{flow_o}", "{out_flo}"], ["{flow}", "{flow}", "{out_flo}", "--bw", "{flow}", "{flow_o}"]):
        refused("chain_flow", argv, files, capsys, named=("flow",), numbers=(W, H))
    assert not any(os.path.exists(files[k]) for k in ("out_png", "out_flo", "out_npz"))


def test_frames_and_guides_that_do_not_fit_the_flow(files, capsys):
    for bad in ("gray_o", "gray_i16"):
        b = "{%s}" % bad
        for argv in (["{gray}", b, "{flow}", "{out_png}"], [b, "{gray}", "{flow}", "{out_png}"], [b, b, "{flow}", "{out_png}"]):
            refused("warp_frame", argv, files, capsys, numbers=(H, W))
        for argv in (["{gray}", b, "{flow}", "{out_npz}"], [b, "{gray}", "{flow}", "{out_npz}"], [b, b, "{flow}", "{out_npz}"]):
            refused("block_motion", argv, files, capsys, named=(bad,), numbers=(H, W))
        refused("filter_flow", ["{flow}", b, "{out_flo}"], files, capsys, named=(bad,), numbers=(H, W))
        refused("motion_blur", [b, "{flow}", "{out_png}"], files, capsys, named=(bad,), numbers=(H, W))
        refused("interp_frame", ["{gray}", b, "0.5", "{out_png}"], files, capsys)
        refused("interp_frame", ["{gray}", "{gray}", "0.5", "{out_png}", "--ref", b], files, capsys)
    refused("interp_frame", ["{gray}", "{gray_f32}", "0.5", "{out_png}"], files, capsys)
    refused("interp_frame", ["{seq}", "{seq}", "0.5", "{out_png}"], files, capsys)            # three-dimensional: not a gray frame
    refused("block_motion", ["{gray_f32}", "{gray_f32}", "{flow}", "{out_npz}"], files, capsys, named=("gray_f32",), numbers=(H, W))
    refused("warp_frame", ["{gray}", "{gray}", "{flow}", "{out_png}", "--occ", "{gray_o}"], files, capsys, numbers=(H, W))
    refused("warp_frame", ["{gray}", "{gray}", "{flow}", "{out_png}", "--occ", "{gray_f32}"], files, capsys, numbers=(H, W))
    assert not any(os.path.exists(files[k]) for k in ("out_png", "out_flo", "out_npz"))


def test_ids_points_and_reference_frames(files, capsys):
    refused("motion_histograms", ["{flow}", "{out_npz}", "--ids", "{ids_i64}"], files, capsys, named=("ids_i64",), numbers=(W, H))
    refused("motion_histograms", ["{flow_o}", "{out_npz}", "--ids", "{gray}"], files, capsys, named=("gray",), numbers=(W + 1, H + 1))
    refused("chain_flow", ["{flow}", "{out_flo}", "--points", "{pts3}", "{traj_npy}"], files, capsys, named=("pts3",))
    refused("chain_flow", ["{flow}", "{out_flo}", "--points", "{gray_f32}", "{traj_npy}"], files, capsys, named=("gray_f32",))
    refused("denoise", ["{seq}", "{out_npy}", "--ref", "{seq_o}"], files, capsys, named=("seq_o",))
    refused("denoise", ["{seq}", "{out_npy}", "--ref", "{seq_c1}"], files, capsys, named=("seq_c1",))
    refused("denoise", ["{seq}", "{out_npy}", "--ref", "{seq_i16}"], files, capsys, named=("seq_i16",))
    assert not any(os.path.exists(files[k]) for k in ("out_npy", "out_flo", "out_npz", "traj_npy"))


class Reached(Exception):
    """the tool accepted its files and asked for a context"""


@pytest.fixture
def contexts(monkeypatch):
    """OFClass replaced by a stand-in that records how it was called and stops the tool there: the list of (op, img, max_batch)"""
    import flowonthego_amd.oflow as oflow
    seen = []

    class OFClass:
        def __init__(self, op, img, max_batch=None):
            seen.append((op, img, max_batch))
            raise Reached

    monkeypatch.setattr(oflow, "OFClass", OFClass)
    return seen


# tool -> (the arguments after frames.npy, the fewest frames it takes, does it take (T, h, w, 1))
SEQUENCE_TOOLS = {"stabilize": (["{out_npy}"], 2, True), "track_objects": (["{out_npz}"], 3, True), "denoise": (["{out_npy}"], 1, True),
                  "motion_blur": (["{out_npy}"], 2, False)}


@pytest.mark.parametrize("tool", sorted(SEQUENCE_TOOLS))
def test_a_frame_sequence_the_tool_cannot_use(tool, files, capsys, contexts):
    tail, fewest, takes_c1 = SEQUENCE_TOOLS[tool]
    for bad in ("seq_i16", "seq_2d", "seq_%d" % (fewest - 1)):
        refused(tool, ["{%s}" % bad] + tail, files, capsys, named=(bad,))
    if not takes_c1:
        refused(tool, ["{seq_c1}"] + tail, files, capsys, named=("seq_c1",))
    assert contexts == []
    with pytest.raises(Reached):
        run(tool, ["{seq_%d}" % fewest] + tail, files, capsys)
    assert len(contexts) == 1


def _context(seen):
    (op, img, max_batch), = seen
    del seen[:]
    return op.channels, op.u8_color, bool(op.bidir), max_batch, img.width, img.height


@pytest.mark.parametrize("tool", sorted(SEQUENCE_TOOLS))
def test_the_context_a_sequence_tool_builds(tool, files, capsys, contexts):
    """8-bit gray and (T, h, w, 1) frames: one channel; 8-bit colour: one channel, made gray from R, G, B on load (u8_color 2);
    float32 colour: three channels.  Both directions and the batch as the tool's feature needs them."""
    tail, _, takes_c1 = SEQUENCE_TOOLS[tool]
    opts = ([], ["--occlusion"]) if tool in ("denoise", "motion_blur") else ([],)
    for opt in opts:
        bidir = True if tool in ("stabilize", "track_objects") else bool(opt)
        batch = {"stabilize": 3, "track_objects": 3, "denoise": 2 * 1 * 4, "motion_blur": 3}[tool]       # four frames in seq*.npy
        forms = {"seq": (1, 0), "seq_rgb": (1, 2), "seq_rgb_f32": (3, 0)}
        if takes_c1:
            forms["seq_c1"] = (1, 0)
        for name, (channels, u8_color) in forms.items():
            with pytest.raises(Reached):
                run(tool, ["{%s}" % name] + tail + opt, files, capsys)
            assert _context(contexts) == (channels, u8_color, bidir, batch, SW, SH), (tool, name, opt)
    if tool == "denoise":                        # the batch follows the radius, and at most eight frames are in flight
        with pytest.raises(Reached):
            run(tool, ["{seq}"] + tail + ["--radius", "3"], files, capsys)
        assert _context(contexts)[3] == 2 * 3 * 4


def test_the_context_interp_frame_builds(files, capsys, contexts):
    with pytest.raises(Reached):
        run("interp_frame", ["{seq_2d}", "{seq_2d}", "0.25", "{out_png}"], files, capsys)
    assert _context(contexts) == (1, 0, True, None, SW, SH)
