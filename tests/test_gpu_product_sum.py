"""Sums of products in the C++ facade (Evaluator::multiply_sum, HybridKeySwitcher::multiply_sum_rescale_range / multiply_sum_lincomb_rescale_range,
ApproxProductSum), through tests/cpp/product_sum/product_sum_words.cpp (a directory of its own below tests/cpp/, as tests/cpp/newton/: built through
tests/cpp_build.py, which makes tests/cpp/bin but no directory below it).

Without a GPU: the program builds and links on tests/cpp/facade_test.h, and its `ref` mode holds the arithmetic of ApproxProductSum::error_bound to the header's
text term by term - and the bound to 2^-10 of max|y| on the float64 reference alone, before any device is asked.
-m gpu, on encrypted inputs at N = 4096 on four data limbs:
* `words`: multiply_sum_rescale_range word for word against the facade's own Evaluator::multiply per pair, summed with Evaluator::add on 3 components, then
  relinearize + rescale; the lincomb form against the same relinearised sum fed to dpfhe_lincomb_rescale with its addend (the identity include/dpfhe.h states for
  the fused second half); terms in {1, 3, 8}, groups in {1, 2}, the second operand per group and shared; the rejections;
* `bound`: ApproxProductSum with terms = 8 and a shared second operand: every decoded slot within error_bound, the bound at most 2^-10 of max|y| >= 1;
* `gate`: the two range methods and ApproxProductSum::apply return while their stream is held (the stream contract of multiply_rescale_range) and give the
  words of the idle stream;
* examples/encrypted_attention_mix_approx at 2 tokens prints OK."""
import os
import re
import subprocess

import pytest

import cpp_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def program():
    os.makedirs(os.path.join(cpp_build.BIN_DIR, "product_sum"), exist_ok=True)
    return cpp_build.build_program("product_sum/product_sum_words", gate=True)


def run(*args, timeout=120):
    return subprocess.run([program(), *args], capture_output=True, text=True, timeout=timeout)


def test_program_links_and_the_bound_arithmetic_holds_without_a_device():
    out = run("ref")
    assert out.returncode == 0 and out.stdout.strip().endswith("product sum reference OK"), out.stdout + out.stderr
    m = re.search(r"max\|y\| ([\d.]+), error_bound 2\^(-?[\d.]+), by hand 2\^(-?[\d.]+)", out.stdout)
    assert m and float(m.group(1)) >= 1.0 and float(m.group(2)) == float(m.group(3)) <= -10.0, out.stdout
    assert run().returncode == 2


@pytest.mark.gpu
def test_words_equal_the_facades_own_products_summed_relinearised_and_rescaled():
    out = run("words")
    assert out.returncode == 0 and out.stdout.strip().endswith("product sum words OK"), out.stdout[-4000:] + out.stderr[-2000:]


@pytest.mark.gpu
def test_encrypted_product_sum_is_within_its_error_bound():
    out = run("bound")
    assert out.returncode == 0 and out.stdout.strip().endswith("product sum bound OK"), out.stdout[-4000:] + out.stderr[-2000:]
    m = re.search(r"max\|y\| ([\d.]+), max error 2\^(-?[\d.]+), error_bound 2\^(-?[\d.]+)", out.stdout)
    assert m and float(m.group(2)) <= float(m.group(3)) <= -10.0 and float(m.group(1)) >= 1.0, out.stdout


@pytest.mark.gpu
def test_facade_calls_only_enqueue_on_their_stream():
    out = run("gate", "0.04")
    assert out.returncode == 0 and out.stdout.strip().endswith("product sum gate OK"), out.stdout[-4000:] + out.stderr[-2000:]


@pytest.mark.gpu
def test_attention_mix_example_prints_ok_at_two_tokens():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "encrypted_attention_mix_approx"])
    out = subprocess.run([os.path.join(ROOT, "examples", "encrypted_attention_mix_approx"), "2", "1", "json"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-4000:] + out.stderr[-2000:]
    assert '"tokens": 2' in out.stdout and '"correct": true' in out.stdout
