! LogLike of the compiled reference's BAO likelihoods (source/bao.f90) at listed
! background values: the recorded outputs of tests/golden/bao/bao_table.tar.xz
! (inputs: tools/bao_make_fixture.py).
!
! The reference's own BAOLikelihood_Add reads use_BAO, bao_dataset[TAG] and the
! bao_dataset[TAG,key] settings from an ini and picks each tag's class (the
! Gaussian, MGSLikelihood, DR1xLikelihood); its own LogLike is called through
! the likelihoods it adds.  The calculator they ask for BAO_D_v,
! AngularDiameterDistance and Hofz_Hunit is a stub that returns the case's
! values whatever the redshift, and Theory%derived_parameters(derived_rdrag) is
! set per case.
!
! Build against the reference objects that build() leaves under oracle/_ref/obj
! (FC, OPENBLAS and OPENBLAS_DIR as in oracle/Makefile; -O2 without fast-math,
! as the oracle's), from the repository root:
!
!   (cd oracle/_ref/obj && $FC -cpp -O2 -w -c ../../../tools/bao_ref_harness.f90 -o bao_ref_harness.o \
!      && objcopy --redefine-syms=../blas.syms bao_ref_harness.o) && \
!   $FC -o oracle/_ref/bao_ref_harness oracle/_ref/obj/bao_ref_harness.o \
!      $(ls oracle/_ref/obj/*.o | grep -v -e harness -e native -e bench) $OPENBLAS -Wl,-rpath,$OPENBLAS_DIR
!
! and run it inside the fixture's directory (the file names of the ini and of
! the datasets are relative to it):
!
!   (cd DIR/bao && ../../oracle/_ref/bao_ref_harness bao.ini cases.txt ref.txt)
!
! cases.txt: ncase / per case one line "k DV DA H rdrag", k the 1-based place of
! the likelihood in the ini's bao_dataset order.  ref.txt receives per case
! "k -lnL" (ES25.17).
module bao_harness_stub
    use settings
    use Calculator_Cosmology
    implicit none

    type, extends(TCosmologyCalculator) :: TStubCalculator
        real(mcp) :: DV = 0, DA = 0, H = 0
    contains
    procedure :: BAO_D_v => Stub_BAO_D_v
    procedure :: AngularDiameterDistance => Stub_AngularDiameterDistance
    procedure :: Hofz_Hunit => Stub_Hofz_Hunit
    end type TStubCalculator

    contains

    real(mcp) function Stub_BAO_D_v(this, z)
    class(TStubCalculator) :: this
    real(mcp), intent(IN) :: z
    Stub_BAO_D_v = this%DV
    end function Stub_BAO_D_v

    real(mcp) function Stub_AngularDiameterDistance(this, z)
    class(TStubCalculator) :: this
    real(mcp), intent(IN) :: z
    Stub_AngularDiameterDistance = this%DA
    end function Stub_AngularDiameterDistance

    real(mcp) function Stub_Hofz_Hunit(this, z)
    class(TStubCalculator) :: this
    real(mcp), intent(IN) :: z
    Stub_Hofz_Hunit = this%H
    end function Stub_Hofz_Hunit

end module bao_harness_stub

program bao_ref_harness
    use settings
    use GeneralTypes
    use CosmologyTypes
    use CosmoTheory
    use Likelihood_Cosmology
    use bao
    use bao_harness_stub
    implicit none
    character(len=512) :: ininame, casefile, outfile
    Type(TSettingIni) :: Ini
    Type(TLikelihoodList) :: List
    Type(TStubCalculator), target :: Stub
    Type(CMBParams) :: CMB
    Type(TCosmoTheoryPredictions), target :: Theory
    class(TDataLikelihood), pointer :: Like
    logical :: bad
    integer :: ncase, i, k, u, uo
    real(mcp) :: v, rd
    real(mcp), allocatable :: nuis(:)

    call get_command_argument(1, ininame)
    call get_command_argument(2, casefile)
    call get_command_argument(3, outfile)
    Feedback = 0
    call Ini%Open(trim(ininame), bad, .false.)
    if (bad) stop 'cannot open the ini'
    call BAOLikelihood_Add(List, Ini)
    if (List%Count < 1) stop 'BAOLikelihood_Add added no likelihood'
    allocate(nuis(0))
    CMB%H0 = 67
    CMB%omv = 0.7_mcp
    CMB%omk = 0
    Theory%derived_parameters = 0

    open(newunit=u, file=trim(casefile), status='old')
    open(newunit=uo, file=trim(outfile), status='replace')
    read(u,*) ncase
    do i = 1, ncase
        read(u,*) k, Stub%DV, Stub%DA, Stub%H, rd
        if (k < 1 .or. k > List%Count) stop 'case names a likelihood that is not there'
        Theory%derived_parameters(derived_rdrag) = rd
        Like => List%Item(k)
        select type (Like)
        class is (TCosmoCalcLikelihood)
            Like%Calculator => Stub
            v = Like%LogLike(CMB, Theory, nuis)
        class default
            stop 'not a TCosmoCalcLikelihood'
        end select
        write(uo,'(I4,ES25.17)') k, v
    end do
    close(uo)
    close(u)
end program
